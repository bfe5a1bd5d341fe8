// iqdemod_spectrum — the band spectrum of one wideband capture file, straight over the C ABI (include/iqdemod.h:
// iqd_spectrum_*): what a user looks at before placing survey points or channels.
//
//   iqdemod_spectrum in=cap.iq rate=2048000 bins=1024 frames=250 format=u8|s8 [window=w.txt] out=power.u32 [log=spectrum.txt]
//                    [detect=runs.txt [rank=512] [ratio_q8=2048] [guard=1] [bridge=8] [minwidth=3] [maxdet=16]
//                     [track=tracks.txt [slots=8] [gate_q8=512] [open=3] [hold=2] [alpha_q8=64] [bias=0] [edges=a,b,c]
//                      [measure=meas.txt [margin=] [beta_q16=328] [carrier=1] [minsum=4096] [carrier_q8=160] [wide=]
//                       [events=events.txt [minactive=2] [votemin=4] [maxevents=256]]]]]
//
//   in       interleaved I/Q, one byte per rail
//   rate     the capture's sample rate in Hz (for the log's offsets only)
//   bins     N: 64, 128, 256, 512, 1024 or 2048
//   frames   F: frames of N samples per block; one spectrum per block
//   format   u8 (offset binary, the default) or s8
//   window   a text file of N int16 values separated by white space or commas; left out: the library's default window
//   out      the API's array, block after block: N little-endian uint32 per block
//   log      one line per block and bin: block, offset in Hz ((k' - N / 2) rate / N), power, dBFS
//   detect   the occupied runs of every block (include/iqdemod.h: "Band activity"), one line per detection: block, the
//            offsets in Hz of its first bin, its last bin and its centroid (iqd_detect_offset_hz), the peak in dBFS,
//            sum_power.  The detector runs on the device straight behind the spectrum, on the same stream.  rate must be
//            a whole number of Hz then.
//   rank ratio_q8 guard bridge minwidth maxdet   iqd_detect_config's floor_rank (left out: bins / 2), ratio_q8, dc_guard,
//            bridge, min_width, max_detections; runs past maxdet per block are counted on stderr
//   track    needs detect=.  The tracker (include/iqdemod.h: "Band tracks") runs on the device behind the detector, on the
//            same stream, with its state carried from one read of the file to the next.  One line per slot record that is
//            live or closing: block, slot, id, state, flags, the centre's offset in Hz (iqd_detect_offset_hz), phase_inc as
//            0x%08x, the offsets in Hz of its first and last bin, class.  Unplaced detections are counted on stderr.
//   slots gate_q8 open hold alpha_q8 bias edges   iqd_track_config's n_slots, gate_q8, open_hits, hold_blocks, alpha_q8,
//            inc_bias, class_edge (left out: bins / 64 + 1, bins / 16, bins / 4 bins)
//   measure  needs track=.  The track measurements (include/iqdemod.h: "Band track measurements") run on the device behind the
//            tracker, on the same stream.  One line per measured record (a live slot): block, slot, id, the offsets in Hz of
//            obw_lo, obw_hi and the peak bin (iqd_detect_offset_hz of the bin's middle, 256 k + 128) and of the centroid,
//            carrier_q8, sum_excess, flags, hint (0 none, 1 carrier, 2 narrow, 3 wide).
//   margin beta_q16 carrier minsum carrier_q8 wide   iqd_measure_config's margin (left out: bins / 256, at least 1),
//            obw_tail_q16, carrier_half, min_sum, carrier_min_q8, wide_bins (left out: bins / 32); dc_guard is guard=
//   events   needs track= and measure=.  The track log (include/iqdemod.h: "Band track log") runs on the device behind the
//            measurements, on the same stream, with its state carried from one read of the file to the next.  One line per
//            event - a track that ended with at least minactive active blocks: id, slot, first block, number of blocks, start
//            time and duration in seconds (blocks of bins x frames samples at rate, %.6f), the mean centre's offset in Hz
//            (iqd_tracklog_mean_centre, iqd_detect_offset_hz; 0 without an active block), the offsets in Hz of obw_lo_min and
//            obw_hi_max (the bin's middle; 0 0 without a voting block), the voted hint (0 none, 1 carrier, 2 narrow, 3 wide),
//            its three vote counts, n_measured, the mean excess power floor(sum_excess / n_measured) (0 without a voting
//            block), flags.  At the end of the input every track still live is read through iqd_tracklog_get_state and written
//            in the same form with the word `open` appended.  Events past maxevents in one call are counted on stderr.
//   minactive votemin maxevents   iqd_tracklog_config's min_active, vote_min, max_events
// A capture that ends inside a block ends with its last whole block; the rest is dropped and counted on stderr.
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

bool readWindow(const std::string &path, std::vector<int16_t> &v)
{
  FILE *f = fopen(path.c_str(), "r");
  if (!f) return false;
  char tok[128];
  bool ok = true;
  while (fscanf(f, " %127[^ \t\r\n,]", tok) == 1) {
    char *end = nullptr;
    const long x = strtol(tok, &end, 10);
    if (*end != 0 || x < -32768 || x > 32767) ok = false;
    v.push_back((int16_t)x);
    int c = fgetc(f);
    if (c != ',' && c != EOF) ungetc(c, f);
  }
  fclose(f);
  return ok && !v.empty();
}

}  // namespace

int main(int argc, char **argv)
{
  std::string in, out, log, windowPath, detectPath, trackPath, measurePath, eventsPath, format = "u8";
  iqd_tracklog_config lc{};
  lc.n_sources = 1;
  lc.max_events = 256;
  lc.min_active = 2;
  lc.vote_min = 4;
  iqd_measure_config mc{};
  mc.n_sources = 1;
  mc.obw_tail_q16 = 328;
  mc.carrier_half = 1;
  mc.min_sum = 4096;
  mc.carrier_min_q8 = 160;
  bool marginGiven = false, wideGiven = false;
  iqd_track_config tc{};
  tc.n_sources = 1;
  tc.n_slots = 8;
  tc.gate_q8 = 512;
  tc.open_hits = 3;
  tc.hold_blocks = 2;
  tc.alpha_q8 = 64;
  bool edgesGiven = false;
  double rate = 0.0;
  uint32_t bins = 0, frames = 0;
  iqd_detect_config dc{};
  dc.ratio_q8 = 2048;
  dc.dc_guard = 1;
  dc.bridge = 8;
  dc.min_width = 3;
  dc.max_detections = 16;
  bool rankGiven = false;
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strncmp(a, "in=", 3)) in = a + 3;
    else if (!strncmp(a, "out=", 4)) out = a + 4;
    else if (!strncmp(a, "log=", 4)) log = a + 4;
    else if (!strncmp(a, "window=", 7)) windowPath = a + 7;
    else if (!strncmp(a, "format=", 7)) format = a + 7;
    else if (!strncmp(a, "rate=", 5)) rate = strtod(a + 5, nullptr);
    else if (!strncmp(a, "bins=", 5)) bins = (uint32_t)strtoul(a + 5, nullptr, 10);
    else if (!strncmp(a, "frames=", 7)) frames = (uint32_t)strtoul(a + 7, nullptr, 10);
    else if (!strncmp(a, "detect=", 7)) detectPath = a + 7;
    else if (!strncmp(a, "rank=", 5)) { dc.floor_rank = (uint32_t)strtoul(a + 5, nullptr, 10); rankGiven = true; }
    else if (!strncmp(a, "ratio_q8=", 9)) dc.ratio_q8 = (uint32_t)strtoul(a + 9, nullptr, 10);
    else if (!strncmp(a, "guard=", 6)) dc.dc_guard = (uint32_t)strtoul(a + 6, nullptr, 10);
    else if (!strncmp(a, "bridge=", 7)) dc.bridge = (uint32_t)strtoul(a + 7, nullptr, 10);
    else if (!strncmp(a, "minwidth=", 9)) dc.min_width = (uint32_t)strtoul(a + 9, nullptr, 10);
    else if (!strncmp(a, "maxdet=", 7)) dc.max_detections = (uint32_t)strtoul(a + 7, nullptr, 10);
    else if (!strncmp(a, "track=", 6)) trackPath = a + 6;
    else if (!strncmp(a, "slots=", 6)) tc.n_slots = (uint32_t)strtoul(a + 6, nullptr, 10);
    else if (!strncmp(a, "gate_q8=", 8)) tc.gate_q8 = (uint32_t)strtoul(a + 8, nullptr, 10);
    else if (!strncmp(a, "open=", 5)) tc.open_hits = (uint32_t)strtoul(a + 5, nullptr, 10);
    else if (!strncmp(a, "hold=", 5)) tc.hold_blocks = (uint32_t)strtoul(a + 5, nullptr, 10);
    else if (!strncmp(a, "alpha_q8=", 9)) tc.alpha_q8 = (uint32_t)strtoul(a + 9, nullptr, 10);
    else if (!strncmp(a, "bias=", 5)) tc.inc_bias = (uint32_t)strtoul(a + 5, nullptr, 0);
    else if (!strncmp(a, "measure=", 8)) measurePath = a + 8;
    else if (!strncmp(a, "margin=", 7)) { mc.margin = (uint32_t)strtoul(a + 7, nullptr, 10); marginGiven = true; }
    else if (!strncmp(a, "beta_q16=", 9)) mc.obw_tail_q16 = (uint32_t)strtoul(a + 9, nullptr, 10);
    else if (!strncmp(a, "carrier=", 8)) mc.carrier_half = (uint32_t)strtoul(a + 8, nullptr, 10);
    else if (!strncmp(a, "minsum=", 7)) mc.min_sum = (uint32_t)strtoul(a + 7, nullptr, 10);
    else if (!strncmp(a, "carrier_q8=", 11)) mc.carrier_min_q8 = (uint32_t)strtoul(a + 11, nullptr, 10);
    else if (!strncmp(a, "wide=", 5)) { mc.wide_bins = (uint32_t)strtoul(a + 5, nullptr, 10); wideGiven = true; }
    else if (!strncmp(a, "events=", 7)) eventsPath = a + 7;
    else if (!strncmp(a, "minactive=", 10)) lc.min_active = (uint32_t)strtoul(a + 10, nullptr, 10);
    else if (!strncmp(a, "votemin=", 8)) lc.vote_min = (uint32_t)strtoul(a + 8, nullptr, 10);
    else if (!strncmp(a, "maxevents=", 10)) lc.max_events = (uint32_t)strtoul(a + 10, nullptr, 10);
    else if (!strncmp(a, "edges=", 6)) {
      edgesGiven = sscanf(a + 6, "%u,%u,%u", &tc.class_edge[0], &tc.class_edge[1], &tc.class_edge[2]) == 3;
      if (!edgesGiven) {
        fprintf(stderr, "iqdemod_spectrum: edges= takes three widths in bins, a,b,c\n");
        return 1;
      }
    }
    else {
      fprintf(stderr, "iqdemod_spectrum: unknown argument %s\n", a);
      return 1;
    }
  }
  const bool u8 = format == "u8";
  if (in.empty() || out.empty() || bins == 0 || frames == 0 || frames > (1u << 24) || !(rate > 0.0) || (!u8 && format != "s8")) {
    fprintf(stderr, "usage: iqdemod_spectrum in=cap.iq rate=2048000 bins=1024 frames=250 format=u8|s8 [window=w.txt] "
                    "out=power.u32 [log=spectrum.txt] [detect=runs.txt [rank=] [ratio_q8=] [guard=] [bridge=] [minwidth=] [maxdet=] "
                    "[track=tracks.txt [slots=] [gate_q8=] [open=] [hold=] [alpha_q8=] [bias=] [edges=a,b,c] "
                    "[measure=meas.txt [margin=] [beta_q16=] [carrier=] [minsum=] [carrier_q8=] [wide=] "
                    "[events=events.txt [minactive=] [votemin=] [maxevents=]]]]]\n");
    return 1;
  }
  const bool detect = !detectPath.empty(), track = !trackPath.empty(), measure = !measurePath.empty(), events = !eventsPath.empty();
  if (events && !(track && measure)) {
    fprintf(stderr, "iqdemod_spectrum: events= needs track= and measure=\n");
    return 1;
  }
  if (measure && !track) {
    fprintf(stderr, "iqdemod_spectrum: measure= needs track=\n");
    return 1;
  }
  if (track && !detect) {
    fprintf(stderr, "iqdemod_spectrum: track= needs detect=\n");
    return 1;
  }
  if (detect && (rate != floor(rate) || rate > 4294967295.0)) {
    fprintf(stderr, "iqdemod_spectrum: detect= needs rate as a whole number of Hz below 2^32\n");
    return 1;
  }
  std::vector<int16_t> window;
  if (!windowPath.empty() && (!readWindow(windowPath, window) || window.size() != bins)) {
    fprintf(stderr, "iqdemod_spectrum: %s does not hold %u int16 values\n", windowPath.c_str(), bins);
    return 1;
  }
  FILE *fin = fopen(in.c_str(), "rb");
  FILE *fout = fin ? fopen(out.c_str(), "wb") : nullptr;
  FILE *flog = fout && !log.empty() ? fopen(log.c_str(), "w") : nullptr;
  FILE *fdet = fout && detect ? fopen(detectPath.c_str(), "w") : nullptr;
  FILE *ftrk = fout && track ? fopen(trackPath.c_str(), "w") : nullptr;
  FILE *fmsr = fout && measure ? fopen(measurePath.c_str(), "w") : nullptr;
  FILE *fevt = fout && events ? fopen(eventsPath.c_str(), "w") : nullptr;
  if (!fin || !fout || (!log.empty() && !flog) || (detect && !fdet) || (track && !ftrk) || (measure && !fmsr) || (events && !fevt)) {
    fprintf(stderr, "iqdemod_spectrum: cannot open the files\n");
    return 1;
  }

  iqd_config cfg{};
  cfg.abi_version = IQD_ABI_VERSION;
  cfg.n_channels = 1;
  cfg.device = -1;
  iqd_t *e = nullptr;
  int rc = iqd_create(&cfg, &e);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_spectrum: iqd_create: %s\n", iqd_strerror(rc));
    return 1;
  }
  iqd_spectrum_config sc{};
  sc.n_sources = 1;
  sc.n_bins = bins;
  sc.window = window.empty() ? nullptr : window.data();
  sc.sample_format = u8 ? IQD_WIDE_U8 : IQD_WIDE_S8;
  iqd_spectrum_t *s = nullptr;
  rc = iqd_spectrum_create(e, &sc, &s);
  uint32_t pfs = 1;
  if (rc == IQD_OK) rc = iqd_spectrum_full_scale(sc.window, bins, &pfs);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_spectrum: iqd_spectrum_create: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
    iqd_destroy(e);
    return 1;
  }

  iqd_detect_t *d = nullptr;
  if (detect) {
    dc.n_bins = bins;
    if (!rankGiven) dc.floor_rank = bins / 2;
    rc = iqd_detect_create(e, &dc, &d);
    if (rc != IQD_OK) {
      fprintf(stderr, "iqdemod_spectrum: iqd_detect_create: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
      iqd_spectrum_destroy(s);
      iqd_destroy(e);
      return 1;
    }
  }

  iqd_track_t *t = nullptr;
  if (track) {
    tc.n_bins = bins;
    tc.max_detections = dc.max_detections;
    if (!edgesGiven) {
      tc.class_edge[0] = bins / 64 + 1;
      tc.class_edge[1] = bins / 16;
      tc.class_edge[2] = bins / 4;
    }
    rc = iqd_track_create(e, &tc, &t);
    if (rc != IQD_OK) {
      fprintf(stderr, "iqdemod_spectrum: iqd_track_create: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
      iqd_detect_destroy(d);
      iqd_spectrum_destroy(s);
      iqd_destroy(e);
      return 1;
    }
  }

  iqd_measure_t *ms = nullptr;
  if (measure) {
    mc.n_bins = bins;
    mc.n_slots = tc.n_slots;
    mc.dc_guard = dc.dc_guard;
    if (!marginGiven) mc.margin = bins / 256 ? bins / 256 : 1;
    if (!wideGiven) mc.wide_bins = bins / 32;
    rc = iqd_measure_create(e, &mc, &ms);
    if (rc != IQD_OK) {
      fprintf(stderr, "iqdemod_spectrum: iqd_measure_create: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
      iqd_track_destroy(t);
      iqd_detect_destroy(d);
      iqd_spectrum_destroy(s);
      iqd_destroy(e);
      return 1;
    }
  }

  iqd_tracklog_t *tl = nullptr;
  if (events) {
    lc.n_slots = tc.n_slots;
    rc = iqd_tracklog_create(e, &lc, &tl);
    if (rc != IQD_OK) {
      fprintf(stderr, "iqdemod_spectrum: iqd_tracklog_create: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
      iqd_measure_destroy(ms);
      iqd_track_destroy(t);
      iqd_detect_destroy(d);
      iqd_spectrum_destroy(s);
      iqd_destroy(e);
      return 1;
    }
  }
  // one line of events=: an event, or a track still live at the end of the input
  auto writeEvent = [&](uint32_t slot, const iqd_track_summary &r, bool open) {
    const double blockSeconds = (double)bins * frames / rate;
    int64_t cen = 0, lo = 0, hi = 0;
    uint32_t mean = 0;
    if (iqd_tracklog_mean_centre(r.sum_centre_q8, r.n_active, &mean) == IQD_OK) iqd_detect_offset_hz(bins, (uint32_t)rate, mean, &cen);
    if (r.n_measured) {
      iqd_detect_offset_hz(bins, (uint32_t)rate, 256u * r.obw_lo_min + 128u, &lo);
      iqd_detect_offset_hz(bins, (uint32_t)rate, 256u * r.obw_hi_max + 128u, &hi);
    }
    fprintf(fevt, "%u %u %llu %u %.6f %.6f %lld %lld %lld %u %u %u %u %u %llu %u%s\n", r.track_id, slot, (unsigned long long)r.first_block,
            r.n_blocks, (double)r.first_block * blockSeconds, (double)r.n_blocks * blockSeconds, (long long)cen, (long long)lo, (long long)hi,
            r.mode_hint, r.votes[0], r.votes[1], r.votes[2], r.n_measured,
            (unsigned long long)(r.n_measured ? r.sum_excess / r.n_measured : 0), r.flags, open ? " open" : "");
  };

  // whole blocks, up to about 16 MiB of capture per call
  const size_t blockBytes = (size_t)2 * bins * frames;
  const size_t perCall = blockBytes >= (16u << 20) ? 1 : (16u << 20) / blockBytes;
  std::vector<uint8_t> buf(perCall * blockBytes);
  std::vector<uint32_t> power(perCall * bins);
  int status = 0;
  uint64_t block = 0, pastMax = 0;
  size_t dropped = 0;
  // detect=: the capture, the power rows and the detector's two arrays stay on the device from one call to the next
  std::vector<iqd_detect_row> rows(detect ? perCall : 0);
  std::vector<iqd_detection> dets(detect ? perCall * dc.max_detections : 0);
  std::vector<iqd_track_slot> slots(track ? perCall * tc.n_slots : 0);
  std::vector<iqd_track_block> tblocks(track ? perCall : 0);
  std::vector<iqd_track_measure> meas(measure ? perCall * tc.n_slots : 0);
  std::vector<iqd_track_summary> evts(events ? lc.max_events : 0);
  // an event record does not say which slot its track sat in: the tool keeps the id every slot of the table showed last
  // (0: none, or closed) and names the slot when the table shows that id ending
  std::vector<uint32_t> slotId(track ? tc.n_slots : 0, 0);
  uint64_t unplaced = 0, eventsPast = 0;
  void *wideDev = nullptr, *powerDev = nullptr, *rowsDev = nullptr, *detDev = nullptr, *slotsDev = nullptr, *tblocksDev = nullptr;
  void *measDev = nullptr, *summaryDev = nullptr, *eventsDev = nullptr, *countsDev = nullptr;
  if (detect) {
    rc = iqd_dev_alloc(e, buf.size(), &wideDev);
    if (rc == IQD_OK) rc = iqd_dev_alloc(e, power.size() * sizeof(uint32_t), &powerDev);
    if (rc == IQD_OK) rc = iqd_dev_alloc(e, rows.size() * sizeof(iqd_detect_row), &rowsDev);
    if (rc == IQD_OK) rc = iqd_dev_alloc(e, dets.size() * sizeof(iqd_detection), &detDev);
    if (rc == IQD_OK && track) rc = iqd_dev_alloc(e, slots.size() * sizeof(iqd_track_slot), &slotsDev);
    if (rc == IQD_OK && track) rc = iqd_dev_alloc(e, tblocks.size() * sizeof(iqd_track_block), &tblocksDev);
    if (rc == IQD_OK && measure) rc = iqd_dev_alloc(e, meas.size() * sizeof(iqd_track_measure), &measDev);
    if (rc == IQD_OK && events) rc = iqd_dev_alloc(e, meas.size() * sizeof(iqd_track_summary), &summaryDev);
    if (rc == IQD_OK && events) rc = iqd_dev_alloc(e, evts.size() * sizeof(iqd_track_summary), &eventsDev);
    if (rc == IQD_OK && events) rc = iqd_dev_alloc(e, sizeof(iqd_tracklog_counts), &countsDev);
    if (rc != IQD_OK) {
      fprintf(stderr, "iqdemod_spectrum: iqd_dev_alloc: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
      iqd_tracklog_destroy(tl);
      iqd_measure_destroy(ms);
      iqd_track_destroy(t);
      iqd_detect_destroy(d);
      iqd_spectrum_destroy(s);
      iqd_destroy(e);
      return 1;
    }
  }
  for (;;) {
    const size_t got = fread(buf.data(), 1, buf.size(), fin);
    const size_t nb = got / blockBytes;
    iqd_tracklog_counts evtCounts{};
    dropped = got - nb * blockBytes;
    if (nb) {
      if (!detect) {
        rc = iqd_spectrum_run(s, buf.data(), nb * blockBytes, frames, power.data());
      } else {
        // spectrum and detector queued back to back on the engine's stream; the host sees the results after both
        rc = iqd_dev_upload(e, wideDev, buf.data(), nb * blockBytes);
        if (rc == IQD_OK) rc = iqd_spectrum_run_device(s, wideDev, nb * blockBytes, frames, (uint32_t *)powerDev);
        if (rc == IQD_OK) rc = iqd_detect_run_device(d, (const uint32_t *)powerDev, nb, (iqd_detect_row *)rowsDev, (iqd_detection *)detDev);
        if (rc == IQD_OK && track)
          rc = iqd_track_run_device(t, (const iqd_detect_row *)rowsDev, (const iqd_detection *)detDev, nb, (iqd_track_slot *)slotsDev,
                                    (iqd_track_block *)tblocksDev);
        if (rc == IQD_OK && measure)
          rc = iqd_measure_run_device(ms, (const uint32_t *)powerDev, (const iqd_detect_row *)rowsDev, (const iqd_track_slot *)slotsDev, nb,
                                      (iqd_track_measure *)measDev);
        if (rc == IQD_OK && events)
          rc = iqd_tracklog_run_device(tl, (const iqd_track_slot *)slotsDev, (const iqd_track_measure *)measDev, nb,
                                       (iqd_track_summary *)summaryDev, (iqd_track_summary *)eventsDev, (iqd_tracklog_counts *)countsDev);
        if (rc == IQD_OK) rc = iqd_dev_download(e, power.data(), powerDev, nb * bins * sizeof(uint32_t));
        if (rc == IQD_OK) rc = iqd_dev_download(e, rows.data(), rowsDev, nb * sizeof(iqd_detect_row));
        if (rc == IQD_OK) rc = iqd_dev_download(e, dets.data(), detDev, nb * dc.max_detections * sizeof(iqd_detection));
        if (rc == IQD_OK && track) rc = iqd_dev_download(e, slots.data(), slotsDev, nb * tc.n_slots * sizeof(iqd_track_slot));
        if (rc == IQD_OK && track) rc = iqd_dev_download(e, tblocks.data(), tblocksDev, nb * sizeof(iqd_track_block));
        if (rc == IQD_OK && measure) rc = iqd_dev_download(e, meas.data(), measDev, nb * tc.n_slots * sizeof(iqd_track_measure));
        if (rc == IQD_OK && events) rc = iqd_dev_download(e, &evtCounts, countsDev, sizeof(evtCounts));
        if (rc == IQD_OK && events && evtCounts.n_stored)
          rc = iqd_dev_download(e, evts.data(), eventsDev, (size_t)evtCounts.n_stored * sizeof(iqd_track_summary));
      }
      if (rc != IQD_OK) {
        fprintf(stderr, "iqdemod_spectrum: %s: %s: %s\n", events ? "spectrum, detector, tracker, measurements and track log" : measure ? "spectrum, detector, tracker and measurements" : track ? "spectrum, detector and tracker" : detect ? "spectrum and detector" : "iqd_spectrum_run", iqd_strerror(rc), iqd_last_error(e));
        status = 3;
        break;
      }
      if (fwrite(power.data(), sizeof(uint32_t), nb * bins, fout) != nb * bins) {
        fprintf(stderr, "iqdemod_spectrum: write failed\n");
        status = 1;
        break;
      }
      for (size_t b = 0; flog && b < nb; b++)
        for (uint32_t k = 0; k < bins; k++) {
          const uint32_t p = power[b * bins + k];
          fprintf(flog, "%llu %.3f %u %.2f\n", (unsigned long long)(block + b), ((double)k - bins / 2) * rate / bins, p,
                  10.0 * log10((double)(p ? p : 1) / (double)(pfs ? pfs : 1)));
        }
      for (size_t b = 0; detect && b < nb; b++) {
        const uint32_t found = rows[b].n_found, shown = found < dc.max_detections ? found : dc.max_detections;
        pastMax += found - shown;
        for (uint32_t i = 0; i < shown; i++) {
          const iqd_detection &r = dets[b * dc.max_detections + i];
          int64_t hz = 0;
          iqd_detect_offset_hz(bins, (uint32_t)rate, r.centroid_q8, &hz);
          fprintf(fdet, "%llu %.3f %.3f %lld %.2f %llu\n", (unsigned long long)(block + b), ((double)r.first_bin - bins / 2) * rate / bins,
                  ((double)r.last_bin - bins / 2) * rate / bins, (long long)hz,
                  10.0 * log10((double)(r.peak_power ? r.peak_power : 1) / (double)(pfs ? pfs : 1)), (unsigned long long)r.sum_power);
        }
      }
      for (size_t b = 0; track && b < nb; b++) {
        unplaced += tblocks[b].n_unplaced;
        for (uint32_t k = 0; k < tc.n_slots; k++) {
          const iqd_track_slot &r = slots[b * tc.n_slots + k];
          if (r.track_id == 0) continue;
          int64_t hz = 0;
          iqd_detect_offset_hz(bins, (uint32_t)rate, r.centre_q8, &hz);
          fprintf(ftrk, "%llu %u %u %u %u %lld 0x%08x %.3f %.3f %u\n", (unsigned long long)(block + b), k, r.track_id, r.state, r.flags,
                  (long long)hz, r.phase_inc, ((double)r.first_bin - bins / 2) * rate / bins, ((double)r.last_bin - bins / 2) * rate / bins,
                  r.width_class);
        }
      }
      for (size_t b = 0; measure && b < nb; b++)
        for (uint32_t k = 0; k < tc.n_slots; k++) {
          const iqd_track_measure &r = meas[b * tc.n_slots + k];
          if (r.track_id == 0) continue;
          int64_t lo = 0, hi = 0, peak = 0, cen = 0;
          iqd_detect_offset_hz(bins, (uint32_t)rate, 256u * r.obw_lo + 128u, &lo);
          iqd_detect_offset_hz(bins, (uint32_t)rate, 256u * r.obw_hi + 128u, &hi);
          iqd_detect_offset_hz(bins, (uint32_t)rate, 256u * r.peak_bin + 128u, &peak);
          iqd_detect_offset_hz(bins, (uint32_t)rate, r.centroid_q8, &cen);
          fprintf(fmsr, "%llu %u %u %lld %lld %lld %lld %u %llu %u %u\n", (unsigned long long)(block + b), k, r.track_id, (long long)lo,
                  (long long)hi, (long long)peak, (long long)cen, r.carrier_q8, (unsigned long long)r.sum_excess, r.flags, r.hint);
        }
      if (events) {
        // events come in block order and within a block in slot order, and so do the table's endings: walk both together
        // (an ending with fewer than minactive active blocks is no event and is passed over; the tracker's ids are unique)
        uint32_t next = 0;
        for (size_t b = 0; b < nb; b++)
          for (uint32_t k = 0; k < tc.n_slots; k++) {
            const iqd_track_slot &r = slots[b * tc.n_slots + k];
            const bool ends = slotId[k] != 0 && (r.track_id != slotId[k] || r.state == 0);
            if (ends && next < evtCounts.n_stored && evts[next].track_id == slotId[k]) writeEvent(k, evts[next++], false);
            slotId[k] = r.state == 0 ? 0 : r.track_id;
          }
        eventsPast += evtCounts.n_events - evtCounts.n_stored;
      }
      block += nb;
    }
    if (got < buf.size()) break;
  }
  if (events && status == 0) {
    // the tracks still live when the input ended
    std::vector<iqd_track_summary> live(tc.n_slots);
    uint64_t g = 0;
    rc = iqd_tracklog_get_state(tl, 0, live.data(), &g);
    if (rc != IQD_OK) {
      fprintf(stderr, "iqdemod_spectrum: iqd_tracklog_get_state: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
      status = 3;
    }
    for (uint32_t k = 0; rc == IQD_OK && k < tc.n_slots; k++)
      if (live[k].track_id != 0) writeEvent(k, live[k], true);
  }
  if (dropped) fprintf(stderr, "iqdemod_spectrum: %zu bytes after the last whole block dropped\n", dropped);
  if (pastMax) fprintf(stderr, "iqdemod_spectrum: %llu runs past maxdet not written\n", (unsigned long long)pastMax);
  if (eventsPast) fprintf(stderr, "iqdemod_spectrum: %llu events past maxevents in their call not written\n", (unsigned long long)eventsPast);
  if (unplaced) fprintf(stderr, "iqdemod_spectrum: %llu detections found no free slot\n", (unsigned long long)unplaced);
  for (void *p : {wideDev, powerDev, rowsDev, detDev, slotsDev, tblocksDev, measDev, summaryDev, eventsDev, countsDev})
    if (p) iqd_dev_free(e, p);
  iqd_tracklog_destroy(tl);
  iqd_measure_destroy(ms);
  iqd_track_destroy(t);
  iqd_detect_destroy(d);
  iqd_spectrum_destroy(s);
  iqd_destroy(e);
  fclose(fin);
  if (fclose(fout) != 0) status = status ? status : 1;
  if (flog && fclose(flog) != 0) status = status ? status : 1;
  if (fdet && fclose(fdet) != 0) status = status ? status : 1;
  if (ftrk && fclose(ftrk) != 0) status = status ? status : 1;
  if (fmsr && fclose(fmsr) != 0) status = status ? status : 1;
  if (fevt && fclose(fevt) != 0) status = status ? status : 1;
  return status;
}
