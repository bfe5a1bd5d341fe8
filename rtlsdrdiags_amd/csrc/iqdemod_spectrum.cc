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

#include "iqd_tool_chain.h"

namespace {

using namespace iqdtool;
const char *const TOOL = "iqdemod_spectrum";

struct Options {
  std::string in, out, log, window, detect, track, measure, events, format = "u8";
  double rate = 0.0;
  uint32_t bins = 0, frames = 0;
  BandArgs band;
  int depth() const { return 1 + !detect.empty() + !track.empty() + !measure.empty() + !events.empty(); }   // (once refusal() passed)
};

// the first thing wrong with the arguments as a whole, as the line to print; nullptr: nothing
const char *refusal(const Options &o)
{
  const bool detect = !o.detect.empty(), track = !o.track.empty(), measure = !o.measure.empty(), events = !o.events.empty();
  if (o.in.empty() || o.out.empty() || o.bins == 0 || o.frames == 0 || o.frames > (1u << 24) || !(o.rate > 0.0) ||
      (o.format != "u8" && o.format != "s8"))
    return "usage: iqdemod_spectrum in=cap.iq rate=2048000 bins=1024 frames=250 format=u8|s8 [window=w.txt] "
           "out=power.u32 [log=spectrum.txt] [detect=runs.txt [rank=] [ratio_q8=] [guard=] [bridge=] [minwidth=] [maxdet=] "
           "[track=tracks.txt [slots=] [gate_q8=] [open=] [hold=] [alpha_q8=] [bias=] [edges=a,b,c] "
           "[measure=meas.txt [margin=] [beta_q16=] [carrier=] [minsum=] [carrier_q8=] [wide=] "
           "[events=events.txt [minactive=] [votemin=] [maxevents=]]]]]\n";
  if (events && !(track && measure)) return "iqdemod_spectrum: events= needs track= and measure=\n";
  if (measure && !track) return "iqdemod_spectrum: measure= needs track=\n";
  if (track && !detect) return "iqdemod_spectrum: track= needs detect=\n";
  if (detect && (o.rate != floor(o.rate) || o.rate > 4294967295.0))
    return "iqdemod_spectrum: detect= needs rate as a whole number of Hz below 2^32\n";
  return nullptr;
}

// what turns bins and powers into the Hz and dBFS of the text files
struct Scale {
  uint32_t bins, frames;
  double rate;
  uint32_t pfs;
  double binHz(uint32_t k) const { return ((double)k - bins / 2) * rate / bins; }
  double dbfs(uint32_t p) const { return 10.0 * log10((double)(p ? p : 1) / (double)(pfs ? pfs : 1)); }
  long long hz(uint32_t q8) const
  {
    int64_t v = 0;
    iqd_detect_offset_hz(bins, (uint32_t)rate, q8, &v);
    return (long long)v;
  }
  long long midHz(uint32_t k) const { return hz(256u * k + 128u); }   // the middle of bin k
};

void writeLog(FILE *f, const Scale &s, uint64_t block, uint32_t k, uint32_t p)
{
  fprintf(f, "%llu %.3f %u %.2f\n", (unsigned long long)block, s.binHz(k), p, s.dbfs(p));
}

void writeDetection(FILE *f, const Scale &s, uint64_t block, const iqd_detection &r)
{
  fprintf(f, "%llu %.3f %.3f %lld %.2f %llu\n", (unsigned long long)block, s.binHz(r.first_bin), s.binHz(r.last_bin), s.hz(r.centroid_q8),
          s.dbfs(r.peak_power), (unsigned long long)r.sum_power);
}

void writeSlot(FILE *f, const Scale &s, uint64_t block, uint32_t k, const iqd_track_slot &r)
{
  fprintf(f, "%llu %u %u %u %u %lld 0x%08x %.3f %.3f %u\n", (unsigned long long)block, k, r.track_id, r.state, r.flags, s.hz(r.centre_q8),
          r.phase_inc, s.binHz(r.first_bin), s.binHz(r.last_bin), r.width_class);
}

void writeMeasure(FILE *f, const Scale &s, uint64_t block, uint32_t k, const iqd_track_measure &r)
{
  fprintf(f, "%llu %u %u %lld %lld %lld %lld %u %llu %u %u\n", (unsigned long long)block, k, r.track_id, s.midHz(r.obw_lo), s.midHz(r.obw_hi),
          s.midHz(r.peak_bin), s.hz(r.centroid_q8), r.carrier_q8, (unsigned long long)r.sum_excess, r.flags, r.hint);
}

// one line of events=: an event, or a track still live at the end of the input
void writeEvent(FILE *f, const Scale &s, uint32_t slot, const iqd_track_summary &r, bool open)
{
  const double blockSeconds = (double)s.bins * s.frames / s.rate;
  uint32_t mean = 0;
  const long long cen = iqd_tracklog_mean_centre(r.sum_centre_q8, r.n_active, &mean) == IQD_OK ? s.hz(mean) : 0;
  const long long lo = r.n_measured ? s.midHz(r.obw_lo_min) : 0, hi = r.n_measured ? s.midHz(r.obw_hi_max) : 0;
  fprintf(f, "%u %u %llu %u %.6f %.6f %lld %lld %lld %u %u %u %u %u %llu %u%s\n", r.track_id, slot, (unsigned long long)r.first_block,
          r.n_blocks, (double)r.first_block * blockSeconds, (double)r.n_blocks * blockSeconds, cen, lo, hi, r.mode_hint, r.votes[0],
          r.votes[1], r.votes[2], r.n_measured, (unsigned long long)(r.n_measured ? r.sum_excess / r.n_measured : 0), r.flags,
          open ? " open" : "");
}

// One call's results on the host, and what the run has counted so far
struct Results {
  std::vector<uint32_t> power;
  std::vector<iqd_detect_row> rows;
  std::vector<iqd_detection> dets;
  std::vector<iqd_track_slot> slots;
  std::vector<iqd_track_block> tblocks;
  std::vector<iqd_track_measure> meas;
  std::vector<iqd_track_summary> evts;
  iqd_tracklog_counts counts{};
  // an event record does not say which slot its track sat in: the tool keeps the id every slot of the table showed last
  // (0: none, or closed) and names the slot when the table shows that id ending
  std::vector<uint32_t> slotId;
  uint64_t block = 0, pastMax = 0, unplaced = 0, eventsPast = 0;
};

// the device arrays' first nb blocks to the host (the first download waits for the stream)
int download(const BandChain &c, const BandArgs &a, size_t nb, Results &r)
{
  int rc = c.power.download(r.power.data(), nb * a.dc.n_bins);
  if (rc == IQD_OK) rc = c.rows.download(r.rows.data(), nb);
  if (rc == IQD_OK) rc = c.det.download(r.dets.data(), nb * a.dc.max_detections);
  if (rc == IQD_OK && c.made >= BandChain::TRACK) rc = c.slots.download(r.slots.data(), nb * a.tc.n_slots);
  if (rc == IQD_OK && c.made >= BandChain::TRACK) rc = c.blocks.download(r.tblocks.data(), nb);
  if (rc == IQD_OK && c.made >= BandChain::MEASURE) rc = c.meas.download(r.meas.data(), nb * a.tc.n_slots);
  if (rc == IQD_OK && c.made >= BandChain::LOG) rc = c.counts.download(&r.counts, 1);
  if (rc == IQD_OK && c.made >= BandChain::LOG && r.counts.n_stored) rc = c.events.download(r.evts.data(), r.counts.n_stored);
  return rc;
}

// the text files' lines of one call of nb blocks
void writeCall(const Scale &s, const BandArgs &a, size_t nb, Results &r, FILE *flog, FILE *fdet, FILE *ftrk, FILE *fmsr, FILE *fevt)
{
  const uint32_t N = s.bins, D = a.dc.max_detections, S = a.tc.n_slots;
  for (size_t b = 0; flog && b < nb; b++)
    for (uint32_t k = 0; k < N; k++) writeLog(flog, s, r.block + b, k, r.power[b * N + k]);
  for (size_t b = 0; fdet && b < nb; b++) {
    const uint32_t found = r.rows[b].n_found, shown = found < D ? found : D;
    r.pastMax += found - shown;
    for (uint32_t i = 0; i < shown; i++) writeDetection(fdet, s, r.block + b, r.dets[b * D + i]);
  }
  for (size_t b = 0; ftrk && b < nb; b++) {
    r.unplaced += r.tblocks[b].n_unplaced;
    for (uint32_t k = 0; k < S; k++)
      if (r.slots[b * S + k].track_id != 0) writeSlot(ftrk, s, r.block + b, k, r.slots[b * S + k]);
  }
  for (size_t b = 0; fmsr && b < nb; b++)
    for (uint32_t k = 0; k < S; k++)
      if (r.meas[b * S + k].track_id != 0) writeMeasure(fmsr, s, r.block + b, k, r.meas[b * S + k]);
  if (!fevt) return;
  // events come in block order and within a block in slot order, and so do the table's endings: walk both together
  // (an ending with fewer than minactive active blocks is no event and is passed over; the tracker's ids are unique)
  uint32_t next = 0;
  for (size_t b = 0; b < nb; b++)
    for (uint32_t k = 0; k < S; k++) {
      const iqd_track_slot &q = r.slots[b * S + k];
      const bool ends = r.slotId[k] != 0 && (q.track_id != r.slotId[k] || q.state == 0);
      if (ends && next < r.counts.n_stored && r.evts[next].track_id == r.slotId[k]) writeEvent(fevt, s, k, r.evts[next++], false);
      r.slotId[k] = q.state == 0 ? 0 : q.track_id;
    }
  r.eventsPast += r.counts.n_events - r.counts.n_stored;
}

}  // namespace

int main(int argc, char **argv)
{
  Options o;
  BandArgs &band = o.band;
  std::vector<Row> keys = {text("in=", o.in), text("out=", o.out), text("log=", o.log), text("window=", o.window), text("format=", o.format),
                           real("rate=", o.rate), u32("bins=", o.bins), u32("frames=", o.frames), text("detect=", o.detect),
                           text("track=", o.track), text("measure=", o.measure), text("events=", o.events)};
  band.rows(keys, TOOL);
  band.logRows(keys);
  if (!parse(argc, argv, keys, TOOL)) return 1;
  if (const char *why = refusal(o)) {
    fputs(why, stderr);
    return 1;
  }
  std::vector<int16_t> window;
  const auto int16 = [](const char *tok, int16_t &x) {
    char *end = nullptr;
    const long v = strtol(tok, &end, 10);
    x = (int16_t)v;
    return *end == 0 && v >= -32768 && v <= 32767;
  };
  if (!o.window.empty() && (!readNumbers(o.window, window, int16) || window.size() != o.bins)) {
    fprintf(stderr, "iqdemod_spectrum: %s does not hold %u int16 values\n", o.window.c_str(), o.bins);
    return 1;
  }
  // the capture, the powers, and one text file per object of the chain that was asked for
  Files files(TOOL);
  FILE *fin = files.open(o.in, "rb", Files::Quiet);
  FILE *fout = fin ? files.open(o.out, "wb", Files::Quiet) : nullptr;
  bool missing = !fout;
  const auto lines = [&](const std::string &path) -> FILE * {
    FILE *f = fout && !path.empty() ? files.open(path, "w", Files::Quiet) : nullptr;
    missing = missing || (!path.empty() && !f);
    return f;
  };
  FILE *flog = lines(o.log), *fdet = lines(o.detect), *ftrk = lines(o.track), *fmsr = lines(o.measure), *fevt = lines(o.events);
  if (missing) {
    fprintf(stderr, "iqdemod_spectrum: cannot open the files\n");
    return 1;
  }

  Engine e;
  int rc = createEngine(e, 1);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_spectrum: iqd_create: %s\n", iqd_strerror(rc));
    return 1;
  }
  const uint32_t bins = o.bins, frames = o.frames;
  const int depth = o.depth();
  const bool detect = depth >= BandChain::DETECT;
  iqd_spectrum_config sc{};
  sc.n_sources = 1;
  sc.n_bins = bins;
  sc.window = window.empty() ? nullptr : window.data();
  sc.sample_format = o.format == "u8" ? IQD_WIDE_U8 : IQD_WIDE_S8;
  band.derive(bins, band.tc.n_slots);
  BandChain chain;
  const char *call = "";
  Scale scale{bins, frames, o.rate, 1};
  rc = chain.create(e, sc, band, BandChain::SPECTRUM, &call);
  if (rc == IQD_OK) rc = iqd_spectrum_full_scale(sc.window, bins, &scale.pfs);
  if (rc == IQD_OK) rc = chain.create(e, sc, band, depth, &call);
  // whole blocks, up to about 16 MiB of capture per call
  const size_t blockBytes = (size_t)2 * bins * frames;
  const size_t perCall = blockBytes >= (16u << 20) ? 1 : (16u << 20) / blockBytes;
  // detect=: the capture, the power rows and the chain's arrays stay on the device from one call to the next
  if (rc == IQD_OK && detect) {
    call = "iqd_dev_alloc";
    rc = chain.alloc(band, perCall, frames);
  }
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_spectrum: %s: %s: %s\n", call, iqd_strerror(rc), iqd_last_error(e));
    return 1;
  }
  const uint32_t S = band.tc.n_slots;
  std::vector<uint8_t> buf(perCall * blockBytes);
  Results r;
  r.power.resize(perCall * bins);
  r.rows.resize(detect ? perCall : 0);
  r.dets.resize(detect ? perCall * band.dc.max_detections : 0);
  r.slots.resize(ftrk ? perCall * S : 0);
  r.tblocks.resize(ftrk ? perCall : 0);
  r.meas.resize(fmsr ? perCall * S : 0);
  r.evts.resize(fevt ? band.lc.max_events : 0);
  r.slotId.assign(ftrk ? S : 0, 0);
  static const char *const what[] = {"", "iqd_spectrum_run", "spectrum and detector", "spectrum, detector and tracker", "spectrum, detector, tracker and measurements",
                                     "spectrum, detector, tracker, measurements and track log"};
  int status = 0;
  size_t dropped = 0;
  for (;;) {
    const size_t got = fread(buf.data(), 1, buf.size(), fin);
    const size_t nb = got / blockBytes;
    dropped = got - nb * blockBytes;
    if (nb) {
      r.counts = iqd_tracklog_counts{};
      if (!detect) rc = iqd_spectrum_run(chain.spectrum, buf.data(), nb * blockBytes, frames, r.power.data());
      else rc = chain.queue(buf.data(), (uint32_t)nb, frames);   // the host sees the results after the whole chain
      if (rc == IQD_OK && detect) rc = download(chain, band, nb, r);
      if (rc != IQD_OK) {
        fprintf(stderr, "iqdemod_spectrum: %s: %s: %s\n", what[depth], iqd_strerror(rc), iqd_last_error(e));
        status = 3;
        break;
      }
      if (fwrite(r.power.data(), sizeof(uint32_t), nb * bins, fout) != nb * bins) {
        fprintf(stderr, "iqdemod_spectrum: write failed\n");
        status = 1;
        break;
      }
      writeCall(scale, band, nb, r, flog, fdet, ftrk, fmsr, fevt);
      r.block += nb;
    }
    if (got < buf.size()) break;
  }
  if (fevt && status == 0) {
    // the tracks still live when the input ended
    std::vector<iqd_track_summary> live(S);
    uint64_t g = 0;
    rc = iqd_tracklog_get_state(chain.tracklog, 0, live.data(), &g);
    if (rc != IQD_OK) {
      fprintf(stderr, "iqdemod_spectrum: iqd_tracklog_get_state: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
      status = 3;
    }
    for (uint32_t k = 0; rc == IQD_OK && k < S; k++)
      if (live[k].track_id != 0) writeEvent(fevt, scale, k, live[k], true);
  }
  if (dropped) fprintf(stderr, "iqdemod_spectrum: %zu bytes after the last whole block dropped\n", dropped);
  if (r.pastMax) fprintf(stderr, "iqdemod_spectrum: %llu runs past maxdet not written\n", (unsigned long long)r.pastMax);
  if (r.eventsPast) fprintf(stderr, "iqdemod_spectrum: %llu events past maxevents in their call not written\n", (unsigned long long)r.eventsPast);
  if (r.unplaced) fprintf(stderr, "iqdemod_spectrum: %llu detections found no free slot\n", (unsigned long long)r.unplaced);
  if (!files.close() && status == 0) status = 1;
  return status;
}
