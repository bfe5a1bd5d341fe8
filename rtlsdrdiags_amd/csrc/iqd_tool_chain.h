// iqd_tool_chain.h — what the command-line tools share of their dealings with the library (the C ABI only): owning handles,
// so that every way out of a tool destroys what it made, in reverse order; and the band chain - spectrum, detector, tracker,
// measurements, track log - with its device arrays and one call's run_device sequence (a new band object is one member of
// BandChain); and what the tools behind a demodulator share: their engine, their PCM input and their tail.
#pragma once
#include "iqd_tool.h"

namespace iqdtool {

template <class T, void (*Destroy)(T *)> struct Handle {
  T *p = nullptr;
  Handle() = default;
  Handle(const Handle &) = delete;
  Handle &operator=(const Handle &) = delete;
  ~Handle() { if (p) Destroy(p); }
  operator T *() const { return p; }
};
using Engine = Handle<iqd_t, iqd_destroy>;
using Channelizer = Handle<iqd_channelizer_t, iqd_channelizer_destroy>;
using Filter = Handle<iqd_filter_t, iqd_filter_destroy>;

// the engine every tool makes: the first usable device
inline int createEngine(Engine &e, uint32_t n_channels, uint32_t block_bytes = 0)
{
  iqd_config cfg{};
  cfg.abi_version = IQD_ABI_VERSION;
  cfg.n_channels = n_channels;
  cfg.block_bytes = block_bytes;
  cfg.device = -1;
  return iqd_create(&cfg, &e.p);
}

// ... as the tools that take PCM make it (iqdemod_tones, iqdemod_fsk), with their line where there is no device
inline bool createPcmEngine(Engine &e, const char *tool)
{
  const int rc = createEngine(e, 1);
  if (rc != IQD_OK) fprintf(stderr, "%s: iqd_create: %s\n", tool, iqd_strerror(rc));
  return rc == IQD_OK;
}

// The PCM those tools read: from stdin (channels = 0) or from the files of a pattern with one %d, chunk samples per channel and call
struct PcmInput {
  std::vector<FILE *> fin;
  std::vector<int16_t> pcm;
  std::vector<uint32_t> count;
  size_t chunk = 0;
  bool more = true;

  // also(c) opens what else the tool keeps per channel, right behind the channel's input; false: Files has said what did not open
  template <class Also> bool open(Files &files, const std::string &pattern, uint32_t channels, size_t chunkSamples, Also also)
  {
    const uint32_t n = channels ? channels : 1;
    chunk = chunkSamples;
    for (uint32_t c = 0; c < n; c++) {
      fin.push_back(channels ? files.open(channelName(pattern, c), "rb", Files::Named) : stdin);
      if (!fin.back() || !also(c)) return false;
    }
    pcm.resize((size_t)n * chunk);
    count.resize(n);
    return true;
  }
  // every channel gives what it has: a channel that has ended counts 0 from then on; got, the call's n, is the longest read.
  // False: nothing is left (a short call was the last)
  bool read(size_t &got)
  {
    got = 0;
    for (size_t c = 0; more && c < fin.size(); c++) {
      const size_t r = fread(pcm.data() + c * chunk, sizeof(int16_t), chunk, fin[c]);
      count[c] = (uint32_t)r;
      if (r > got) got = r;
    }
    more = got == chunk;
    return got != 0;
  }
};

// the tail of those tools: what went to stdout or to the files is out, or the status, if still 0, is 1
inline int closeOutputs(Files &files, int status)
{
  const bool flushed = fflush(stdout) == 0;
  return (!files.close() || !flushed) && status == 0 ? 1 : status;
}

// n elements of T in device memory (Free = iqd_dev_free) or in page-locked host memory (iqd_host_free)
template <class T, int (*Free)(iqd_t *, void *) = iqd_dev_free> struct Buffer {
  iqd_t *e = nullptr;
  T *p = nullptr;
  Buffer() = default;
  Buffer(const Buffer &) = delete;
  Buffer &operator=(const Buffer &) = delete;
  ~Buffer() { if (p) Free(e, p); }
  int alloc(iqd_t *engine, size_t n, int (*how)(iqd_t *, size_t, void **) = iqd_dev_alloc)
  {
    void *raw = nullptr;
    const int rc = how(e = engine, n * sizeof(T), &raw);
    p = (T *)raw;
    return rc;
  }
  int download(T *dst, size_t n) const { return iqd_dev_download(e, dst, p, n * sizeof(T)); }
  operator T *() const { return p; }
};
template <class T> using HostBuffer = Buffer<T, iqd_host_free>;

struct BandChain {
  enum Depth { SPECTRUM = 1, DETECT, TRACK, MEASURE, LOG };
  iqd_t *e = nullptr;
  int made = 0;   // the objects that exist: a Depth
  size_t bins = 0;
  // (members are destroyed last to first: the arrays, then the objects from the track log back to the spectrum)
  Handle<iqd_spectrum_t, iqd_spectrum_destroy> spectrum;
  Handle<iqd_detect_t, iqd_detect_destroy> detect;
  Handle<iqd_track_t, iqd_track_destroy> track;
  Handle<iqd_measure_t, iqd_measure_destroy> measure;
  Handle<iqd_tracklog_t, iqd_tracklog_destroy> tracklog;
  Buffer<uint8_t> wide;
  Buffer<uint32_t> power;
  Buffer<iqd_detect_row> rows;
  Buffer<iqd_detection> det;
  Buffer<iqd_track_slot> slots;
  Buffer<iqd_track_block> blocks;
  Buffer<iqd_track_measure> meas;
  Buffer<iqd_track_summary> summary, events;
  Buffer<iqd_tracklog_counts> counts;

  // creates the objects from `made` up to `depth`; on a refusal *failed names the call
  int create(iqd_t *engine, const iqd_spectrum_config &sc, const BandArgs &a, int depth, const char **failed)
  {
    e = engine;
    int rc = IQD_OK;
    while (rc == IQD_OK && made < depth) {
      switch (made + 1) {
        case SPECTRUM: *failed = "iqd_spectrum_create"; rc = iqd_spectrum_create(e, &sc, &spectrum.p); break;
        case DETECT: *failed = "iqd_detect_create"; rc = iqd_detect_create(e, &a.dc, &detect.p); break;
        case TRACK: *failed = "iqd_track_create"; rc = iqd_track_create(e, &a.tc, &track.p); break;
        case MEASURE: *failed = "iqd_measure_create"; rc = iqd_measure_create(e, &a.mc, &measure.p); break;
        default: *failed = "iqd_tracklog_create"; rc = iqd_tracklog_create(e, &a.lc, &tracklog.p); break;
      }
      if (rc == IQD_OK) made++;
    }
    return rc;
  }
  // the device arrays of a call of up to K blocks of bins x frames samples
  int alloc(const BandArgs &a, size_t K, uint32_t frames)
  {
    const size_t N = bins = a.dc.n_bins, S = a.tc.n_slots;
    int rc = wide.alloc(e, K * 2 * N * frames);
    if (rc == IQD_OK) rc = power.alloc(e, K * N);
    if (rc == IQD_OK) rc = rows.alloc(e, K);
    if (rc == IQD_OK) rc = det.alloc(e, K * a.dc.max_detections);
    if (rc == IQD_OK && made >= TRACK) rc = slots.alloc(e, K * S);
    if (rc == IQD_OK && made >= TRACK) rc = blocks.alloc(e, K);
    if (rc == IQD_OK && made >= MEASURE) rc = meas.alloc(e, K * S);
    if (rc == IQD_OK && made >= LOG) rc = summary.alloc(e, K * S);
    if (rc == IQD_OK && made >= LOG) rc = events.alloc(e, a.lc.max_events);
    if (rc == IQD_OK && made >= LOG) rc = counts.alloc(e, 1);
    return rc;
  }
  // one call: nb blocks go up and every object is queued behind the one before it on the engine's stream; nothing waits
  int queue(const uint8_t *host, uint32_t nb, uint32_t frames)
  {
    const size_t bytes = (size_t)nb * 2 * bins * frames;
    int rc = iqd_dev_upload(e, wide, host, bytes);
    if (rc == IQD_OK) rc = iqd_spectrum_run_device(spectrum, wide, bytes, frames, power);
    if (rc == IQD_OK) rc = iqd_detect_run_device(detect, power, nb, rows, det);
    if (rc == IQD_OK && made >= TRACK) rc = iqd_track_run_device(track, rows, det, nb, slots, blocks);
    if (rc == IQD_OK && made >= MEASURE) rc = iqd_measure_run_device(measure, power, rows, slots, nb, meas);
    if (rc == IQD_OK && made >= LOG) rc = iqd_tracklog_run_device(tracklog, slots, meas, nb, summary, events, counts);
    return rc;
  }
};

}  // namespace iqdtool
