// iqdemod_wide — many channels out of ONE wideband capture, straight over the C ABI (include/iqdemod.h): the one-receiver
// counterpart of iqdemod_multi.  The capture is interleaved I/Q (uint8, or format=s8 / s16) at decimation x 256 kS/s (an RTL-SDR at 2.048 MS/s
// is decimation=8, one at 2.4 MS/s decimation=75/8); every channel is cut out by the channelizer (iqd_channelizer_*) at its offset from the capture's
// centre and demodulated by one engine channel - one reference IqDataProcessor with its demodulators (Radio.cc:150-181).
// PCM goes out as S16_LE at 8 kS/s (radioApp.cc:103-111), one file per channel.
//
//   iqdemod_wide in=cap.iq [decimation=8] rate=2048000 offsets=<Hz>[,<Hz>...] modes=<m>[,<m>...] [gains=<L>[,<L>...]]
//                out=pcm_%d.s16 [blocks=K] [rotation=<r>] [centre=<Hz>] [scan=<start>,<end>,<step>[,...]]
//                [squelch=<dBFS>[,<dBFS>...]] [freqlog=<file>]
//                [survey=<first_offset_Hz>,<step_Hz>,<count> [surveyshift=<L>] surveylog=<file>] [format=u8|s8|s16]
//                [agc=off|lowpass|harris[,...]] [rxgain=<dB>[,<dB>...]] [gainlog=<file>]
//   iqdemod_wide in=cap.iq rate=2048000 tracks=<S> bins=<N> frames=<F> modes=<m>[,...] [gains=<L>[,...]] out=pcm_%d.s16
//                [blocks=K] [lag=0|1] [minstate=1|2] [tracklog=<file>] [squelch=<dBFS>[,...]]
//                [rank=] [ratio_q8=] [guard=] [bridge=] [minwidth=] [maxdet=] [gate_q8=] [open=] [hold=] [alpha_q8=] [bias=] [edges=a,b,c]
//                [measlog=<file>] [margin=] [beta_q16=] [carrier=] [minsum=] [carrier_q8=] [wide=]      (and modes=auto)
//
//   format     what the capture holds: u8 offset binary (an RTL-SDR; the default), s8 signed int8 (hackrf_transfer), s16
//              little-endian signed int16 (SDRplay, Airspy, USRP, SDR++ / SDR# / SDRangel basebands).  s8 and s16 are for
//              fixed channels at an integer decimation: not together with survey=, scan= or a fractional rate.
//   decimation M, or P/Q with Q = 2, 4 or 8 (rate = 256000 P / Q); left out, it is rate / 256000 in lowest terms
//   offsets    the channel's frequency minus the capture's centre, Hz (|offset| < rate / 2)
//   modes      per channel, the list repeating (0 none 1 am 2 fm 3 wbfm 4 lsb 5 usb)
//   gains      the channelizer's gain shift L per channel, 0..8 (6 dB each), the list repeating; default 0
//   rotation   the engine's Fs/4 selector for every channel (+1, the reference's default, wants each offset at
//              station + 64 kHz, like the reference's tuning, Radio.cc:617-618; 0 wants it on the station)
//   blocks     32768-byte engine blocks per channel and call (default 4); a capture that ends inside a call ends with
//              its whole blocks and then the rest, cut to a multiple of 64 x decimation (64 P) bytes, as one short block
//   centre     the capture's centre frequency, Hz (default 0): where scanning channels find their stations
//   scan       per channel a scan grid of station frequencies, Hz (FrequencyScanner::setScanParameters, then start()),
//              the triplets repeating like modes; such a channel follows its scanner (iqd_channelizer_follow_scanner):
//              every block is cut at the frequency the scanner held when it began.  A triplet 0,0,0 leaves the channel
//              at its offset.
//   squelch    per channel the squelch threshold, dBFS, the list repeating (default: the engine's)
//   freqlog    one line per block and channel: block (from 0, over the whole capture), channel, the station frequency
//              the block was cut at (a fixed channel: centre + offset - 64000 rotation), 1 if the squelch let it through
//   agc        per channel its AutomaticGainControl, the list repeating: off (the default), lowpass or harris.  A channel
//              with a running AGC follows its gain (iqd_channelizer_follow_gain): the channelizer applies the channel's IF
//              gain in dB to every block in place of gains=, so the AGC levels the channel.
//   rxgain     per channel the IF gain in dB (iqd_set_rx_gain_db), the list repeating; every channel then follows its gain
//              (with agc=off it is the channel's manual gain).  agc= and rxgain= are for a u8 capture at an integer
//              decimation and not together with scan=.
//   gainlog    one line per block and channel: block (from 0, over the whole capture), channel, the gain in dB the block
//              was cut with (a channel that does not follow its gain: 6 L)
//   survey     a grid of count offsets first, first + step, ... (the increments as for offsets; count <= 4096): every
//              accept is surveyed before it is run (iqd_channelizer_survey, one block per 32768-byte engine block, the
//              short block at the capture's end as one block - left out, with a notice, where its length is no admissible
//              survey block).  surveylog gets one line per block and point: block (from 0, over the whole capture), the
//              point's offset in Hz, the block magnitude, its level in dBFS (iqd_magnitude_dbfs; no gain applied).
//              surveyshift: the gain shift L of every point (default 0).  With survey=, offsets= (and modes=, out=) may
//              be left out: then nothing is demodulated and no PCM files are written.  Not together with scan=.
//   tracks     S channels that follow the band's tracks (include/iqdemod.h: "Track-following channels") in place of
//              offsets=: per call of K table blocks (blocks=, default 4; a table block is bins x frames samples) the band
//              spectrum, the activity detector, the tracker and the channelizer's accept are queued on one stream, and
//              channel s is cut at slot s of the tracker's table, block by block.  bins, frames and the detector's and
//              tracker's keys are iqdemod_spectrum's, with its defaults (tracks= stands for slots=); bias= is the tracker's
//              inc_bias and the engine channels' rotation is 0 (the tracker's centre is the station itself).  lag, minstate:
//              iqd_track_follow's (defaults 0 and 2).  2 bins frames / decimation, the row bytes of a table block, must be a
//              multiple of 256 and at most 32768 (it is the engine's block), or K of them together.  A capture that ends
//              inside a call ends with its whole table blocks as one shorter call; a trailing part that does not fill a
//              table block is dropped and counted on stderr.  Not together with scan=, agc= / rxgain=, a fractional rate or
//              format=s8|s16.
//   tracklog   one line per table block and channel: block (from 0, over the whole capture), channel, 1 if the block was
//              cut (live) else 0, the phase_inc it was cut with as 0x%08x, and that increment as an offset in Hz
//   modes=auto with tracks=: every channel starts as FM and the track measurements (include/iqdemod.h: "Band track
//              measurements"; the keys margin ... wide are iqdemod_spectrum's, with its defaults) are queued behind the tracker
//              in every call.  After a call the tool looks, per slot, at the track_id the slot has in the call's last block
//              in which it is active: if it has not decided for that id yet, it takes the hint that most of the call's blocks
//              in which this id is active give (ties go to the lowest hint; blocks without a hint do not vote) and sets
//              the channel's mode with iqd_set_mode - CARRIER am, NARROW fm, WIDE wbfm, no hint at all fm.  THE MODE IS IN
//              FORCE FROM THE NEXT CALL ON - a lag of one call (blocks= table blocks): the call that first sees a track
//              active is still demodulated with the mode the channel had.  The mode then stays while that track_id lives.
//              The hint is a hint: an unmodulated FM carrier looks like am, a sideband signal like fm.
//   measlog    tracks= only, with or without modes=auto.  One line per measured record: "m", block (from 0, over the whole
//              capture), slot, id, flags, hint, obw_hi - obw_lo + 1 in bins, carrier_q8, sum_excess; and one line per mode
//              the tool sets: "mode", the first block of the call that decided it, slot, id, the mode (1 am 2 fm 3 wbfm).
// Exit status 0, 1 (no device / bad arguments / I/O), 3 (a call was rejected).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "iqdemod.h"

namespace {

std::vector<double> numList(const char *s)
{
  std::vector<double> v;
  for (const char *q = s; *q;) {
    v.push_back(atof(q));
    const char *c = strchr(q, ',');
    if (!c) break;
    q = c + 1;
  }
  return v;
}

std::vector<uint64_t> u64List(const char *s)
{
  std::vector<uint64_t> v;
  for (const char *q = s; *q;) {
    v.push_back(strtoull(q, nullptr, 10));
    const char *c = strchr(q, ',');
    if (!c) break;
    q = c + 1;
  }
  return v;
}

struct TrackArgs {
  std::string in, out, tracklog, measlog;
  iqd_measure_config mc{};
  bool autoModes = false, marginGiven = false, wideGiven = false;
  uint32_t m = 0, S = 0, bins = 0, frames = 0, blocks = 4, lag = 0, minstate = 2;
  double rate = 0;
  std::vector<double> modes, gains, squelch;
  iqd_detect_config dc{};
  iqd_track_config tc{};
  bool rankGiven = false, edgesGiven = false;
};

// tracks=: spectrum -> detector -> tracker -> accept_wideband on one stream per call, one synchronise (the downloads)
int runTracks(const TrackArgs &a)
{
  const uint32_t n = a.S, N = a.bins, F = a.frames, M = a.m;
  const size_t wide_block = (size_t)2 * N * F;             // capture bytes of one table block
  const size_t bb = wide_block / M;                        // its row bytes
  if (wide_block % M != 0 || bb % 64 != 0) {
    fprintf(stderr, "iqdemod_wide: tracks= needs 2 bins frames / decimation to be a multiple of 64\n");
    return 1;
  }
  uint32_t engine_bb = 0;
  if (bb % 256 == 0 && bb <= 32768) engine_bb = (uint32_t)bb;
  else if (a.blocks * bb % 256 == 0 && a.blocks * bb <= 32768) engine_bb = (uint32_t)(a.blocks * bb);
  if (!engine_bb) {
    fprintf(stderr, "iqdemod_wide: tracks= needs 2 bins frames / decimation (or blocks= of them) to be a multiple of 256, at most 32768\n");
    return 1;
  }
  FILE *f = fopen(a.in.c_str(), "rb");
  if (!f) {
    fprintf(stderr, "iqdemod_wide: cannot open %s\n", a.in.c_str());
    return 1;
  }
  std::vector<FILE *> sinks(n);
  for (uint32_t c = 0; c < n; c++) {
    char name[4096];
    snprintf(name, sizeof(name), a.out.c_str(), (int)c);
    if (!(sinks[c] = fopen(name, "wb"))) {
      fprintf(stderr, "iqdemod_wide: cannot create %s\n", name);
      return 1;
    }
  }
  FILE *tlog = nullptr;
  if (!a.tracklog.empty() && !(tlog = fopen(a.tracklog.c_str(), "w"))) {
    fprintf(stderr, "iqdemod_wide: cannot create %s\n", a.tracklog.c_str());
    return 1;
  }
  iqd_config cfg{};
  cfg.abi_version = IQD_ABI_VERSION;
  cfg.n_channels = n;
  cfg.block_bytes = engine_bb;
  cfg.device = -1;
  iqd_t *e = nullptr;
  int rc = iqd_create(&cfg, &e);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_wide: iqd_create: %s\n", iqd_strerror(rc));
    return 1;
  }
  iqd_spectrum_config sc{};
  sc.n_sources = 1;
  sc.n_bins = N;
  iqd_detect_config dc = a.dc;
  dc.n_bins = N;
  if (!a.rankGiven) dc.floor_rank = N / 2;
  iqd_track_config tc = a.tc;
  tc.n_sources = 1;
  tc.n_bins = N;
  tc.n_slots = n;
  tc.max_detections = dc.max_detections;
  if (!a.edgesGiven) {
    tc.class_edge[0] = N / 64 + 1;
    tc.class_edge[1] = N / 16;
    tc.class_edge[2] = N / 4;
  }
  const bool measuring = a.autoModes || !a.measlog.empty();
  iqd_measure_config mc = a.mc;
  mc.n_sources = 1;
  mc.n_bins = N;
  mc.n_slots = n;
  mc.dc_guard = dc.dc_guard;
  if (!a.marginGiven) mc.margin = N / 256 ? N / 256 : 1;
  if (!a.wideGiven) mc.wide_bins = N / 32;
  iqd_measure_t *ms = nullptr;
  FILE *mlog = nullptr;
  if (!a.measlog.empty() && !(mlog = fopen(a.measlog.c_str(), "w"))) {
    fprintf(stderr, "iqdemod_wide: cannot create %s\n", a.measlog.c_str());
    return 1;
  }
  iqd_channelizer_config zc{};
  zc.n_sources = 1;
  zc.n_channels = n;
  zc.decimation = M;
  iqd_spectrum_t *s = nullptr;
  iqd_detect_t *d = nullptr;
  iqd_track_t *t = nullptr;
  iqd_channelizer_t *z = nullptr;
  rc = iqd_spectrum_create(e, &sc, &s);
  if (rc == IQD_OK) rc = iqd_detect_create(e, &dc, &d);
  if (rc == IQD_OK) rc = iqd_track_create(e, &tc, &t);
  if (rc == IQD_OK && measuring) rc = iqd_measure_create(e, &mc, &ms);
  if (rc == IQD_OK) rc = iqd_channelizer_create(e, &zc, &z);
  std::vector<uint32_t> source(n, 0), inc(n, 0);
  std::vector<uint8_t> shift(n);
  std::vector<int32_t> slot(n);
  for (uint32_t c = 0; c < n; c++) {
    shift[c] = (uint8_t)a.gains[c % a.gains.size()];
    slot[c] = (int32_t)c;
  }
  if (rc == IQD_OK) rc = iqd_channelizer_set_channels(z, 0, n, source.data(), inc.data(), shift.data());
  if (rc == IQD_OK) rc = iqd_channelizer_follow_tracks(z, 0, n, slot.data());
  for (uint32_t c = 0; c < n && rc == IQD_OK; c++) rc = iqd_set_mode(e, c, 1, (int)a.modes[c % a.modes.size()]);
  if (rc == IQD_OK) rc = iqd_set_rotation(e, 0, n, 0);
  for (uint32_t c = 0; c < n && rc == IQD_OK && !a.squelch.empty(); c++)
    rc = iqd_set_squelch(e, c, 1, (int32_t)a.squelch[c % a.squelch.size()]);
  const uint32_t K = a.blocks, D = dc.max_detections;
  const size_t call = K * wide_block, row = K * bb;
  void *d_wide = nullptr, *d_pow = nullptr, *d_rows = nullptr, *d_det = nullptr, *d_slots = nullptr, *d_blocks = nullptr;
  void *d_out = nullptr, *d_pcm = nullptr, *d_cnt = nullptr, *d_meas = nullptr;
  if (rc == IQD_OK) rc = iqd_dev_alloc(e, call, &d_wide);
  if (rc == IQD_OK) rc = iqd_dev_alloc(e, (size_t)K * N * 4, &d_pow);
  if (rc == IQD_OK) rc = iqd_dev_alloc(e, (size_t)K * sizeof(iqd_detect_row), &d_rows);
  if (rc == IQD_OK) rc = iqd_dev_alloc(e, (size_t)K * D * sizeof(iqd_detection), &d_det);
  if (rc == IQD_OK) rc = iqd_dev_alloc(e, (size_t)K * n * sizeof(iqd_track_slot), &d_slots);
  if (rc == IQD_OK) rc = iqd_dev_alloc(e, (size_t)K * sizeof(iqd_track_block), &d_blocks);
  if (rc == IQD_OK) rc = iqd_dev_alloc(e, (size_t)n * row, &d_out);
  if (rc == IQD_OK) rc = iqd_dev_alloc(e, (size_t)n * (row / 64) * 2, &d_pcm);
  if (rc == IQD_OK) rc = iqd_dev_alloc(e, (size_t)n * 4, &d_cnt);
  if (rc == IQD_OK && measuring) rc = iqd_dev_alloc(e, (size_t)K * n * sizeof(iqd_track_measure), &d_meas);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_wide: setup: %s (%s)\n", iqd_strerror(rc), iqd_last_error(e));
    return 1;
  }
  std::vector<uint8_t> wide(call);
  std::vector<int16_t> pcm((size_t)n * (row / 64));
  std::vector<uint32_t> count(n);
  std::vector<iqd_track_slot> slots((size_t)K * n);
  std::vector<uint32_t> carry_live(n, 0), carry_inc(n, 0);   // the tool's copy of the followers' carries, for the log
  std::vector<iqd_track_measure> meas(measuring ? (size_t)K * n : 0);
  std::vector<uint32_t> decided(n, 0);                       // modes=auto: the track_id each channel's mode was chosen for
  std::vector<int> current(n);
  for (uint32_t c = 0; c < n; c++) current[c] = (int)a.modes[c % a.modes.size()];
  uint64_t block_no = 0;
  size_t dropped = 0;
  int status = 0;
  for (;;) {
    const size_t got = fread(wide.data(), 1, call, f);
    const uint32_t nb = (uint32_t)(got / wide_block);
    dropped += got - nb * wide_block;
    if (nb == 0) break;
    const size_t bytes = nb * wide_block, r_bytes = nb * bb;
    iqd_track_follow tf{};
    tf.slots_dev = (const iqd_track_slot *)d_slots;
    tf.n_slots = n;
    tf.n_blocks = nb;
    tf.block_bytes = (uint32_t)bb;
    tf.lag = a.lag;
    tf.min_state = a.minstate;
    int r = iqd_dev_upload(e, d_wide, wide.data(), bytes);
    if (r == IQD_OK) r = iqd_spectrum_run_device(s, d_wide, bytes, F, (uint32_t *)d_pow);
    if (r == IQD_OK) r = iqd_detect_run_device(d, (const uint32_t *)d_pow, nb, (iqd_detect_row *)d_rows, (iqd_detection *)d_det);
    if (r == IQD_OK) r = iqd_track_run_device(t, (const iqd_detect_row *)d_rows, (const iqd_detection *)d_det, nb,
                                              (iqd_track_slot *)d_slots, (iqd_track_block *)d_blocks);
    if (r == IQD_OK && measuring)
      r = iqd_measure_run_device(ms, (const uint32_t *)d_pow, (const iqd_detect_row *)d_rows, (const iqd_track_slot *)d_slots, nb,
                                 (iqd_track_measure *)d_meas);
    if (r == IQD_OK) r = iqd_channelizer_set_track_table(z, &tf);
    if (r == IQD_OK) r = iqd_accept_wideband_device(e, z, 0, d_wide, bytes, d_out, d_pcm, d_cnt, nullptr, nullptr);
    if (r == IQD_OK) r = iqd_synchronize(e);
    if (r == IQD_OK) r = iqd_dev_download(e, pcm.data(), d_pcm, (size_t)n * (r_bytes / 64) * 2);
    if (r == IQD_OK) r = iqd_dev_download(e, count.data(), d_cnt, (size_t)n * 4);
    if (r == IQD_OK && (tlog || measuring)) r = iqd_dev_download(e, slots.data(), d_slots, (size_t)nb * n * sizeof(iqd_track_slot));
    if (r == IQD_OK && measuring) r = iqd_dev_download(e, meas.data(), d_meas, (size_t)nb * n * sizeof(iqd_track_measure));
    if (r != IQD_OK) {
      fprintf(stderr, "iqdemod_wide: tracks: %s (%s)\n", iqd_strerror(r), iqd_last_error(e));
      status = 3;
      break;
    }
    for (uint32_t c = 0; c < n; c++)
      if (fwrite(&pcm[(size_t)c * (r_bytes / 64)], 2, count[c], sinks[c]) != count[c]) {
        fprintf(stderr, "iqdemod_wide: write failed\n");
        status = 1;
      }
    if (tlog) {
      auto decide = [&](uint32_t b, uint32_t c, uint32_t &live, uint32_t &d_inc) {
        const iqd_track_slot &q = slots[(size_t)b * n + c];
        live = q.state >= a.minstate ? 1u : 0u;
        d_inc = live ? q.phase_inc : 0u;
      };
      for (uint32_t b = 0; b < nb; b++)
        for (uint32_t c = 0; c < n; c++) {
          uint32_t live = carry_live[c], d_inc = carry_inc[c];
          if (b >= a.lag) decide(b - a.lag, c, live, d_inc);
          fprintf(tlog, "%llu %u %u 0x%08x %lld\n", (unsigned long long)(block_no + b), c, live, d_inc,
                  (long long)llround((double)(int32_t)d_inc / 4294967296.0 * a.rate));
        }
      for (uint32_t c = 0; c < n; c++) decide(nb - 1, c, carry_live[c], carry_inc[c]);
    }
    for (uint32_t b = 0; mlog && b < nb; b++)
      for (uint32_t c = 0; c < n; c++) {
        const iqd_track_measure &q = meas[(size_t)b * n + c];
        if (q.track_id)
          fprintf(mlog, "m %llu %u %u %u %u %u %u %llu\n", (unsigned long long)(block_no + b), c, q.track_id, q.flags, q.hint,
                  q.flags & IQD_MEASURE_F_EMPTY ? 0u : q.obw_hi - q.obw_lo + 1u, q.carrier_q8, (unsigned long long)q.sum_excess);
      }
    for (uint32_t c = 0; a.autoModes && c < n && status == 0; c++) {
      uint32_t id = 0;
      for (uint32_t b = 0; b < nb; b++)
        if (slots[(size_t)b * n + c].state == IQD_TRACK_ACTIVE) id = slots[(size_t)b * n + c].track_id;
      if (id == 0 || id == decided[c]) continue;
      uint32_t votes[4] = {0, 0, 0, 0};
      for (uint32_t b = 0; b < nb; b++) {
        const iqd_track_slot &q = slots[(size_t)b * n + c];
        if (q.state == IQD_TRACK_ACTIVE && q.track_id == id) votes[meas[(size_t)b * n + c].hint & 3]++;
      }
      uint32_t hint = IQD_HINT_NONE;
      for (uint32_t h = IQD_HINT_CARRIER; h <= IQD_HINT_WIDE; h++)
        if (votes[h] > (hint ? votes[hint] : 0u)) hint = h;
      const int mode = hint == IQD_HINT_CARRIER ? 1 : hint == IQD_HINT_WIDE ? 3 : 2;
      const int r2 = mode == current[c] ? IQD_OK : iqd_set_mode(e, c, 1, mode);   // (a channel that has the mode is left alone)
      current[c] = mode;
      if (r2 != IQD_OK) {
        fprintf(stderr, "iqdemod_wide: iqd_set_mode: %s (%s)\n", iqd_strerror(r2), iqd_last_error(e));
        status = 3;
        break;
      }
      decided[c] = id;
      if (mlog) fprintf(mlog, "mode %llu %u %u %d\n", (unsigned long long)block_no, c, id, mode);
    }
    if (status == 3) break;
    block_no += nb;
    if (got < call) break;
  }
  if (dropped) fprintf(stderr, "iqdemod_wide: %zu trailing bytes do not fill a table block: dropped\n", dropped);
  fclose(f);
  if (tlog) fclose(tlog);
  if (mlog) fclose(mlog);
  for (FILE *q : sinks) fclose(q);
  iqd_channelizer_destroy(z);
  iqd_measure_destroy(ms);
  iqd_track_destroy(t);
  iqd_detect_destroy(d);
  iqd_spectrum_destroy(s);
  iqd_destroy(e);
  return status;
}

}  // namespace

int main(int argc, char **argv)
{
  TrackArgs ta;
  ta.dc.ratio_q8 = 2048;
  ta.dc.dc_guard = 1;
  ta.dc.bridge = 8;
  ta.dc.min_width = 3;
  ta.dc.max_detections = 16;
  ta.tc.gate_q8 = 512;
  ta.tc.open_hits = 3;
  ta.tc.hold_blocks = 2;
  ta.tc.alpha_q8 = 64;
  ta.mc.obw_tail_q16 = 328;
  ta.mc.carrier_half = 1;
  ta.mc.min_sum = 4096;
  ta.mc.carrier_min_q8 = 160;
  std::string in, out, freqlog, surveylog, gainlog;
  uint32_t m = 0, den = 1, blocks = 4;
  bool m_given = false;
  double rate = 0;
  int rotation = 1;
  uint64_t centre = 0;
  std::vector<double> offsets, modes, gains{0}, squelch, rxgain;
  std::vector<std::string> agc;
  std::vector<uint64_t> scan;
  std::vector<double> survey;
  uint32_t surveyshift = 0;
  std::string format = "u8";
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strncmp(a, "in=", 3)) in = a + 3;
    else if (!strncmp(a, "out=", 4)) out = a + 4;
    else if (!strncmp(a, "decimation=", 11)) {
      m = (uint32_t)atoi(a + 11);
      const char *slash = strchr(a + 11, '/');
      den = slash ? (uint32_t)atoi(slash + 1) : 1;
      m_given = true;
    }
    else if (!strncmp(a, "rate=", 5)) rate = atof(a + 5);
    else if (!strncmp(a, "offsets=", 8)) offsets = numList(a + 8);
    else if (!strcmp(a, "modes=auto")) { ta.autoModes = true; modes = {2.0}; }
    else if (!strncmp(a, "modes=", 6)) modes = numList(a + 6);
    else if (!strncmp(a, "gains=", 6)) gains = numList(a + 6);
    else if (!strncmp(a, "blocks=", 7)) blocks = (uint32_t)atoi(a + 7);
    else if (!strncmp(a, "rotation=", 9)) rotation = atoi(a + 9);
    else if (!strncmp(a, "centre=", 7)) centre = strtoull(a + 7, nullptr, 10);
    else if (!strncmp(a, "scan=", 5)) scan = u64List(a + 5);
    else if (!strncmp(a, "squelch=", 8)) squelch = numList(a + 8);
    else if (!strncmp(a, "freqlog=", 8)) freqlog = a + 8;
    else if (!strncmp(a, "survey=", 7)) survey = numList(a + 7);
    else if (!strncmp(a, "surveyshift=", 12)) surveyshift = (uint32_t)atoi(a + 12);
    else if (!strncmp(a, "surveylog=", 10)) surveylog = a + 10;
    else if (!strncmp(a, "format=", 7)) format = a + 7;
    else if (!strncmp(a, "rxgain=", 7)) rxgain = numList(a + 7);
    else if (!strncmp(a, "gainlog=", 8)) gainlog = a + 8;
    else if (!strncmp(a, "tracks=", 7)) ta.S = (uint32_t)strtoul(a + 7, nullptr, 10);
    else if (!strncmp(a, "bins=", 5)) ta.bins = (uint32_t)strtoul(a + 5, nullptr, 10);
    else if (!strncmp(a, "frames=", 7)) ta.frames = (uint32_t)strtoul(a + 7, nullptr, 10);
    else if (!strncmp(a, "lag=", 4)) ta.lag = (uint32_t)strtoul(a + 4, nullptr, 10);
    else if (!strncmp(a, "minstate=", 9)) ta.minstate = (uint32_t)strtoul(a + 9, nullptr, 10);
    else if (!strncmp(a, "tracklog=", 9)) ta.tracklog = a + 9;
    else if (!strncmp(a, "measlog=", 8)) ta.measlog = a + 8;
    else if (!strncmp(a, "margin=", 7)) { ta.mc.margin = (uint32_t)strtoul(a + 7, nullptr, 10); ta.marginGiven = true; }
    else if (!strncmp(a, "beta_q16=", 9)) ta.mc.obw_tail_q16 = (uint32_t)strtoul(a + 9, nullptr, 10);
    else if (!strncmp(a, "carrier=", 8)) ta.mc.carrier_half = (uint32_t)strtoul(a + 8, nullptr, 10);
    else if (!strncmp(a, "minsum=", 7)) ta.mc.min_sum = (uint32_t)strtoul(a + 7, nullptr, 10);
    else if (!strncmp(a, "carrier_q8=", 11)) ta.mc.carrier_min_q8 = (uint32_t)strtoul(a + 11, nullptr, 10);
    else if (!strncmp(a, "wide=", 5)) { ta.mc.wide_bins = (uint32_t)strtoul(a + 5, nullptr, 10); ta.wideGiven = true; }
    else if (!strncmp(a, "rank=", 5)) { ta.dc.floor_rank = (uint32_t)strtoul(a + 5, nullptr, 10); ta.rankGiven = true; }
    else if (!strncmp(a, "ratio_q8=", 9)) ta.dc.ratio_q8 = (uint32_t)strtoul(a + 9, nullptr, 10);
    else if (!strncmp(a, "guard=", 6)) ta.dc.dc_guard = (uint32_t)strtoul(a + 6, nullptr, 10);
    else if (!strncmp(a, "bridge=", 7)) ta.dc.bridge = (uint32_t)strtoul(a + 7, nullptr, 10);
    else if (!strncmp(a, "minwidth=", 9)) ta.dc.min_width = (uint32_t)strtoul(a + 9, nullptr, 10);
    else if (!strncmp(a, "maxdet=", 7)) ta.dc.max_detections = (uint32_t)strtoul(a + 7, nullptr, 10);
    else if (!strncmp(a, "gate_q8=", 8)) ta.tc.gate_q8 = (uint32_t)strtoul(a + 8, nullptr, 10);
    else if (!strncmp(a, "open=", 5)) ta.tc.open_hits = (uint32_t)strtoul(a + 5, nullptr, 10);
    else if (!strncmp(a, "hold=", 5)) ta.tc.hold_blocks = (uint32_t)strtoul(a + 5, nullptr, 10);
    else if (!strncmp(a, "alpha_q8=", 9)) ta.tc.alpha_q8 = (uint32_t)strtoul(a + 9, nullptr, 10);
    else if (!strncmp(a, "bias=", 5)) ta.tc.inc_bias = (uint32_t)strtoul(a + 5, nullptr, 0);
    else if (!strncmp(a, "edges=", 6)) {
      ta.edgesGiven = sscanf(a + 6, "%u,%u,%u", &ta.tc.class_edge[0], &ta.tc.class_edge[1], &ta.tc.class_edge[2]) == 3;
      if (!ta.edgesGiven) {
        fprintf(stderr, "iqdemod_wide: edges= takes three widths in bins, a,b,c\n");
        return 1;
      }
    }
    else if (!strncmp(a, "agc=", 4)) {
      for (const char *q = a + 4;;) {
        const char *c = strchr(q, ',');
        agc.push_back(c ? std::string(q, c) : std::string(q));
        if (!c) break;
        q = c + 1;
      }
    }
    else {
      fprintf(stderr, "iqdemod_wide: unknown argument %s\n", a);
      return 1;
    }
  }
  if (!m_given && rate > 0) {   // rate / 256000 = P / Q in lowest terms
    const double r8 = rate / 32000.0;
    if (r8 != floor(r8) || r8 < 16 || r8 > 512) {
      fprintf(stderr, "iqdemod_wide: rate must be 256000 P / Q with Q = 1, 2, 4 or 8 and 2 <= P / Q <= 64 (or give decimation=P/Q)\n");
      return 1;
    }
    m = (uint32_t)r8;
    den = 8;
    while (den > 1 && m % 2 == 0) {
      m /= 2;
      den /= 2;
    }
  }
  if (format != "u8" && format != "s8" && format != "s16") {
    fprintf(stderr, "iqdemod_wide: format must be u8, s8 or s16\n");
    return 1;
  }
  const uint32_t sample_format = format == "s16" ? IQD_WIDE_S16 : format == "s8" ? IQD_WIDE_S8 : IQD_WIDE_U8;
  const size_t rail = format == "s16" ? 2 : 1;   // bytes per rail
  if (sample_format != IQD_WIDE_U8 && (!survey.empty() || !scan.empty() || den > 1)) {
    fprintf(stderr, "iqdemod_wide: format=%s cannot be combined with %s: not built for signed captures yet\n", format.c_str(),
            !survey.empty() ? "survey=" : !scan.empty() ? "scan=" : "a fractional rate");
    return 1;
  }
  bool gain_following = !rxgain.empty();
  for (const std::string &t : agc) {
    if (t != "off" && t != "lowpass" && t != "harris") {
      fprintf(stderr, "iqdemod_wide: agc must be off, lowpass or harris\n");
      return 1;
    }
    gain_following = gain_following || t != "off";
  }
  if (gain_following && (!scan.empty() || den > 1 || sample_format != IQD_WIDE_U8)) {
    fprintf(stderr, "iqdemod_wide: agc= / rxgain= cannot be combined with %s: channels that follow their gain are not built for it yet\n",
            !scan.empty() ? "scan=" : den > 1 ? "a fractional rate" : "format=s8|s16");
    return 1;
  }
  if (!ta.S && (ta.autoModes || !ta.measlog.empty())) {
    fprintf(stderr, "iqdemod_wide: modes=auto and measlog= need tracks=\n");
    return 1;
  }
  if (ta.S) {
    if (!scan.empty() || gain_following || den > 1 || sample_format != IQD_WIDE_U8) {
      fprintf(stderr, "iqdemod_wide: tracks= cannot be combined with %s: channels that follow tracks are not built for it yet\n",
              !scan.empty() ? "scan=" : gain_following ? "agc= / rxgain=" : den > 1 ? "a fractional rate" : "format=s8|s16");
      return 1;
    }
    if (in.empty() || out.empty() || modes.empty() || gains.empty() || m < 2 || rate <= 0 || !blocks || ta.S > 64 || !ta.bins ||
        !ta.frames || ta.lag > 1 || ta.minstate < 1 || ta.minstate > 2 || !offsets.empty() || !survey.empty()) {
      fprintf(stderr, "usage: iqdemod_wide in=cap.iq rate=2048000 tracks=S(1..64) bins=N frames=F modes=<m,...> [gains=<L,...>] "
                      "out=pcm_%%d.s16 [blocks=K] [lag=0|1] [minstate=1|2] [tracklog=file] [squelch=dBFS,...] [rank=] [ratio_q8=] "
                      "[measlog=file] [margin=] [beta_q16=] [carrier=] [minsum=] [carrier_q8=] [wide=] "
                      "[guard=] [bridge=] [minwidth=] [maxdet=] [gate_q8=] [open=] [hold=] [alpha_q8=] [bias=] [edges=a,b,c]\n"
                      "  (not with offsets=, survey=, scan=, agc=, rxgain=, a fractional rate or format=s8|s16; the capture's whole table\n"
                      "  blocks of bins x frames samples are run, a trailing part that does not fill one is dropped and counted;\n"
                      "  modes=auto: every channel starts as fm, and the mode chosen from a track's measured hints - carrier am,\n"
                      "  narrow fm, wide wbfm - is in force from the call AFTER the one that first sees the track active: a lag of\n"
                      "  one call)\n");
      return 1;
    }
    ta.in = in;
    ta.out = out;
    ta.m = m;
    ta.rate = rate;
    ta.blocks = blocks;
    ta.modes = modes;
    ta.gains = gains;
    ta.squelch = squelch;
    return runTracks(ta);
  }
  const bool surveying = !survey.empty();
  const bool survey_ok = !surveying || (survey.size() == 3 && survey[2] >= 1 && survey[2] <= 4096 && surveyshift <= 8 && !surveylog.empty());
  const bool demod_ok = !offsets.empty() ? !out.empty() && !modes.empty() : surveying;
  if (surveying && !scan.empty()) {   // (iqd_channelizer_survey refuses while a channel follows its scanner)
    fprintf(stderr, "iqdemod_wide: survey= cannot be combined with scan=: a survey is refused while a channel follows its scanner\n");
    return 1;
  }
  if (in.empty() || !demod_ok || !survey_ok || m < 2 || den < 1 || rate <= 0 || gains.empty() || !blocks || scan.size() % 3 != 0) {
    fprintf(stderr, "usage: iqdemod_wide in=cap.iq [decimation=8|75/8] rate=2048000 offsets=<Hz,...> modes=<m,...> "
                    "[gains=<L,...>] out=pcm_%%d.s16 [blocks=K] [rotation=r] [centre=Hz] [scan=start,end,step,...] "
                    "[squelch=dBFS,...] [freqlog=file] [survey=first_Hz,step_Hz,count [surveyshift=L] surveylog=file] [format=u8|s8|s16] "
                    "[agc=off|lowpass|harris,...] [rxgain=dB,...] [gainlog=file]\n");
    return 1;
  }
  const uint32_t n = (uint32_t)offsets.size();   // 0: survey only
  const uint32_t n_pts = surveying ? (uint32_t)survey[2] : 0;
  std::vector<uint32_t> sv_inc(n_pts);
  std::vector<uint8_t> sv_shift(n_pts, (uint8_t)surveyshift);
  std::vector<double> sv_off(n_pts);
  for (uint32_t p = 0; p < n_pts; p++) {
    sv_off[p] = survey[0] + p * survey[1];
    if (fabs(sv_off[p]) >= rate / 2) {
      fprintf(stderr, "iqdemod_wide: survey offset %.0f Hz outside +-rate/2\n", sv_off[p]);
      return 1;
    }
    sv_inc[p] = (uint32_t)(int32_t)llround(sv_off[p] / rate * 4294967296.0);
  }
  std::vector<uint32_t> source(n, 0), inc(n);
  std::vector<uint8_t> shift(n);
  for (uint32_t c = 0; c < n; c++) {
    if (fabs(offsets[c]) >= rate / 2) {
      fprintf(stderr, "iqdemod_wide: offset %.0f Hz outside +-rate/2\n", offsets[c]);
      return 1;
    }
    // f_c = int32(d_c) / 2^32 * rate
    inc[c] = (uint32_t)(int32_t)llround(offsets[c] / rate * 4294967296.0);
    shift[c] = (uint8_t)gains[c % gains.size()];
  }

  FILE *f = fopen(in.c_str(), "rb");
  if (!f) {
    fprintf(stderr, "iqdemod_wide: cannot open %s\n", in.c_str());
    return 1;
  }
  std::vector<FILE *> sinks(n);
  for (uint32_t c = 0; c < n; c++) {
    char name[4096];
    snprintf(name, sizeof(name), out.c_str(), (int)c);
    sinks[c] = fopen(name, "wb");
    if (!sinks[c]) {
      fprintf(stderr, "iqdemod_wide: cannot create %s\n", name);
      return 1;
    }
  }
  FILE *slog = nullptr;
  if (surveying && !(slog = fopen(surveylog.c_str(), "w"))) {
    fprintf(stderr, "iqdemod_wide: cannot create %s\n", surveylog.c_str());
    return 1;
  }
  FILE *flog = nullptr;
  if (!freqlog.empty() && !(flog = fopen(freqlog.c_str(), "w"))) {
    fprintf(stderr, "iqdemod_wide: cannot create %s\n", freqlog.c_str());
    return 1;
  }

  FILE *glog = nullptr;
  if (!gainlog.empty() && !(glog = fopen(gainlog.c_str(), "w"))) {
    fprintf(stderr, "iqdemod_wide: cannot create %s\n", gainlog.c_str());
    return 1;
  }

  iqd_config cfg{};
  cfg.abi_version = IQD_ABI_VERSION;
  cfg.n_channels = n ? n : 1;
  cfg.device = -1;
  iqd_t *e = nullptr;
  int rc = iqd_create(&cfg, &e);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_wide: iqd_create: %s\n", iqd_strerror(rc));
    return 1;
  }
  iqd_channelizer_config zc{};
  zc.n_sources = 1;
  zc.n_channels = n ? n : 1;   // (survey only: one channel at offset 0 carries the stream's history along)
  zc.decimation = m;
  zc.decimation_den = den;
  zc.sample_format = sample_format;
  iqd_channelizer_t *z = nullptr;
  rc = iqd_channelizer_create(e, &zc, &z);
  if (rc == IQD_OK && n) rc = iqd_channelizer_set_channels(z, 0, n, source.data(), inc.data(), shift.data());
  if (rc == IQD_OK && surveying) rc = iqd_channelizer_set_survey(z, n_pts, sv_inc.data(), sv_shift.data());
  for (uint32_t c = 0; c < n && rc == IQD_OK; c++) rc = iqd_set_mode(e, c, 1, (int)modes[c % modes.size()]);
  if (rc == IQD_OK && n) rc = iqd_set_rotation(e, 0, n, rotation);
  for (uint32_t c = 0; c < n && rc == IQD_OK && !squelch.empty(); c++)
    rc = iqd_set_squelch(e, c, 1, (int32_t)squelch[c % squelch.size()]);
  // scanning channels: their scanners and the channelizer's following flags
  std::vector<uint8_t> follows(n, 0);
  if (rc == IQD_OK) rc = iqd_channelizer_set_source_frequency(z, 0, 1, &centre);
  for (uint32_t c = 0; c < n && rc == IQD_OK && !scan.empty(); c++) {
    const uint64_t *g = &scan[3 * (c % (scan.size() / 3))];
    if (!g[0] && !g[1] && !g[2]) continue;
    rc = iqd_scanner_set_parameters(e, c, 1, g[0], g[1], g[2]);
    if (rc == IQD_OK) rc = iqd_scanner_start(e, c, 1, 1);
    if (rc == IQD_OK) rc = iqd_channelizer_follow_scanner(z, c, 1, 1);
    follows[c] = 1;
  }
  // channels that follow their gain: a running AGC, or a gain in dB of their own
  std::vector<uint8_t> follows_gain(n, 0);
  for (uint32_t c = 0; c < n && rc == IQD_OK; c++) {
    const std::string t = agc.empty() ? "off" : agc[c % agc.size()];
    if (!rxgain.empty()) rc = iqd_set_rx_gain_db(e, c, 1, (uint32_t)rxgain[c % rxgain.size()]);
    if (rc == IQD_OK && t != "off") rc = iqd_agc_set_type(e, c, 1, t == "harris" ? IQD_AGC_HARRIS : IQD_AGC_LOWPASS);
    if (rc == IQD_OK && t != "off") rc = iqd_agc_enable(e, c, 1, 1);
    follows_gain[c] = t != "off" || !rxgain.empty();
    if (rc == IQD_OK && follows_gain[c]) rc = iqd_channelizer_follow_gain(z, c, 1, 1);
  }
  if (rc == IQD_OK && glog) rc = iqd_set_gain_trace(e, 1);
  std::vector<uint32_t> gtrace;
  // the frequency each channel's next block is cut at: the scanner's (its start() jump applied), or the fixed one
  std::vector<uint64_t> cut(n), trace;
  if (rc == IQD_OK && flog) rc = iqd_set_gain_trace(e, 1);
  for (uint32_t c = 0; c < n && rc == IQD_OK && flog; c++) {
    if (follows[c]) rc = iqd_scanner_get(e, c, &cut[c], nullptr, nullptr);
    else cut[c] = (uint64_t)((int64_t)centre + llround(offsets[c]) - 64000 * (int64_t)rotation);
  }
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_wide: setup: %s (%s)\n", iqd_strerror(rc), iqd_last_error(e));
    return 1;
  }

  // (wide bytes per engine block: 32768 m / den = 64 m (512 / den), whole calls of the channelizer)
  // (rail bytes per rail: a signed 16-bit capture has twice the bytes per block; den is 1 there)
  const size_t block = 32768 / den * (size_t)m * rail, call = blocks * block, unit = 64 * (size_t)m * rail;
  std::vector<uint8_t> wide(call);
  std::vector<int16_t> pcm((size_t)n * call / m / rail * den / 64);
  std::vector<uint32_t> sv_mag((size_t)blocks * n_pts);
  std::vector<uint8_t> sv_rows(n ? 0 : call / m * den);
  std::vector<uint32_t> count(n);
  std::vector<uint8_t> open((size_t)n * blocks);
  uint64_t block_no = 0;
  int status = 0;
  // one accept of `bytes` (whole engine blocks, or ONE short block: include/iqdemod.h), its PCM and its log lines out
  auto feed = [&](const uint8_t *p, size_t bytes) {
    const size_t nblk = bytes % block == 0 ? bytes / block : 1;
    int r = IQD_OK;
    if (surveying) {   // before the run: a survey reads the state the accept starts from
      const size_t bb = bytes / m * den / nblk;   // row bytes per block
      if (bb % (den > 1 ? 256 : 64) != 0) {
        fprintf(stderr, "iqdemod_wide: the short block of %zu row bytes is not surveyed\n", bb);
      } else {
        r = iqd_channelizer_survey(z, p, bytes, (uint32_t)bb, sv_mag.data());
        for (size_t b = 0; r == IQD_OK && b < nblk; b++)
          for (uint32_t q = 0; q < n_pts; q++) {
            const uint32_t mg = sv_mag[b * n_pts + q];
            fprintf(slog, "%llu %lld %u %d\n", (unsigned long long)(block_no + b), (long long)llround(sv_off[q]), mg,
                    (int)iqd_magnitude_dbfs(mg));
          }
      }
    }
    // survey only: nothing is demodulated, but the stream moves on - the one channel at offset 0 is run (its row comes
    // back to the host and is dropped: 1 / M of the capture's bytes, the price of advancing the history over the C ABI)
    if (r == IQD_OK && !n) {
      r = iqd_channelizer_run(z, p, bytes, sv_rows.data());
      if (r != IQD_OK) {
        fprintf(stderr, "iqdemod_wide: survey: %s (%s)\n", iqd_strerror(r), iqd_last_error(e));
        status = 3;
        return false;
      }
      block_no += nblk;
      return true;
    }
    if (r == IQD_OK) r = iqd_accept_wideband(e, z, 0, p, bytes, pcm.data(), count.data(), nullptr, flog ? open.data() : nullptr);
    if (r == IQD_OK && flog) {
      trace.resize((size_t)n * nblk);
      r = iqd_get_frequency_trace(e, 0, n, trace.data(), nblk);
    }
    if (r == IQD_OK && glog) {
      gtrace.resize((size_t)n * nblk);
      r = iqd_get_gain_trace(e, 0, n, gtrace.data(), nblk);
    }
    if (r != IQD_OK) {
      fprintf(stderr, "iqdemod_wide: accept: %s (%s)\n", iqd_strerror(r), iqd_last_error(e));
      status = 3;
      return false;
    }
    const size_t row = bytes / m / rail * den / 64;
    for (uint32_t c = 0; c < n; c++)
      if (fwrite(&pcm[(size_t)c * row], 2, count[c], sinks[c]) != count[c]) {
        fprintf(stderr, "iqdemod_wide: write failed\n");
        status = 1;
      }
    for (size_t b = 0; flog && b < nblk; b++)
      for (uint32_t c = 0; c < n; c++) {
        fprintf(flog, "%llu %u %llu %u\n", (unsigned long long)(block_no + b), c, (unsigned long long)cut[c],
                (unsigned)open[(size_t)c * nblk + b]);
        if (follows[c]) cut[c] = trace[(size_t)c * nblk + b];   // the frequency after this block's scanner step
      }
    for (size_t b = 0; glog && b < nblk; b++)
      for (uint32_t c = 0; c < n; c++) {
        const uint32_t g = gtrace[(size_t)c * nblk + b];
        fprintf(glog, "%llu %u %u\n", (unsigned long long)(block_no + b), c,
                follows_gain[c] ? (g < IQD_GAIN_FOLLOW_MAX ? g : (uint32_t)IQD_GAIN_FOLLOW_MAX) : 6u * shift[c]);
      }
    block_no += nblk;
    return true;
  };
  for (;;) {
    size_t got = fread(wide.data(), 1, call, f);
    got -= got % unit;
    if (got == 0) break;
    // a capture that ends inside a call: its whole blocks first, then the rest as one short block
    const size_t whole = got / block * block, rest = got - whole;
    if (whole && !feed(wide.data(), whole)) break;
    if (rest && !feed(wide.data() + whole, rest)) break;
    if (got < call) break;
  }
  fclose(f);
  if (flog) fclose(flog);
  if (slog) fclose(slog);
  if (glog) fclose(glog);
  for (FILE *s : sinks) fclose(s);
  iqd_channelizer_destroy(z);
  iqd_destroy(e);
  return status;
}
