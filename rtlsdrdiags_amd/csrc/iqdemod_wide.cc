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
#include <stdarg.h>

#include "iqd_tool_chain.h"

namespace {

using namespace iqdtool;
const char *const TOOL = "iqdemod_wide";

struct Options {
  std::string in, out, freqlog, surveylog, gainlog, tracklog, measlog, format = "u8";
  uint32_t m = 0, den = 1, blocks = 4, surveyshift = 0, tracks = 0, bins = 0, frames = 0, lag = 0, minstate = 2;
  bool mGiven = false, autoModes = false;
  double rate = 0;
  int rotation = 1;
  uint64_t centre = 0;
  std::vector<double> offsets, modes, gains{0}, squelch, rxgain, survey;
  std::vector<std::string> agc;
  std::vector<uint64_t> scan;
  BandArgs band;
  uint32_t sampleFormat = IQD_WIDE_U8;   // (format=, once refusal() has passed it)

  std::vector<Row> keys()
  {
    std::vector<Row> t = {
        text("in=", in), text("out=", out), real("rate=", rate), viaAtoi("blocks=", blocks), viaAtoi("rotation=", rotation),
        {"decimation=", [this](const char *v) {   // P[/Q]
           const char *slash = strchr(v, '/');
           m = (uint32_t)atoi(v);
           den = slash ? (uint32_t)atoi(slash + 1) : 1;
           return true;
         }, &mGiven},
        {"offsets=", [this](const char *v) { offsets = doubleList(v); return true; }},
        word("modes=auto", [this] { autoModes = true; modes = {2.0}; }),
        {"modes=", [this](const char *v) { modes = doubleList(v); return true; }},
        {"gains=", [this](const char *v) { gains = doubleList(v); return true; }},
        viaStrtoull("centre=", centre),
        {"scan=", [this](const char *v) { scan = u64List(v); return true; }},
        {"squelch=", [this](const char *v) { squelch = doubleList(v); return true; }},
        text("freqlog=", freqlog),
        {"survey=", [this](const char *v) { survey = doubleList(v); return true; }},
        viaAtoi("surveyshift=", surveyshift), text("surveylog=", surveylog), text("format=", format),
        {"rxgain=", [this](const char *v) { rxgain = doubleList(v); return true; }},
        text("gainlog=", gainlog),
        {"agc=", [this](const char *v) {   // (given twice, the names add up)
           for (const std::string &t : nameList(v)) agc.push_back(t);
           return true;
         }},
        u32("tracks=", tracks), u32("bins=", bins), u32("frames=", frames), u32("lag=", lag), u32("minstate=", minstate),
        text("tracklog=", tracklog), text("measlog=", measlog)};
    band.rows(t, TOOL);
    return t;
  }
  template <class T> static T of(const std::vector<T> &list, uint32_t c) { return list[c % list.size()]; }   // the list repeating
};

std::string say(const char *fmt, ...)
{
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}

// f_c = int32(d_c) / 2^32 * rate
uint32_t incOf(double offset, double rate) { return (uint32_t)(int32_t)llround(offset / rate * 4294967296.0); }
long long hzOf(uint32_t inc, double rate) { return (long long)llround((double)(int32_t)inc / 4294967296.0 * rate); }

// tracks=: the engine's block - a table block's row bytes, or blocks= of them; 0: neither will do
uint32_t trackEngineBlock(const Options &o)
{
  const size_t bb = (size_t)2 * o.bins * o.frames / o.m;
  if (bb % 256 == 0 && bb <= 32768) return (uint32_t)bb;
  if (o.blocks * bb % 256 == 0 && o.blocks * bb <= 32768) return (uint32_t)(o.blocks * bb);
  return 0;
}

const char *const USAGE =
    "usage: iqdemod_wide in=cap.iq [decimation=8|75/8] rate=2048000 offsets=<Hz,...> modes=<m,...> "
    "[gains=<L,...>] out=pcm_%d.s16 [blocks=K] [rotation=r] [centre=Hz] [scan=start,end,step,...] "
    "[squelch=dBFS,...] [freqlog=file] [survey=first_Hz,step_Hz,count [surveyshift=L] surveylog=file] [format=u8|s8|s16] "
    "[agc=off|lowpass|harris,...] [rxgain=dB,...] [gainlog=file]\n";
const char *const TRACKS_USAGE =
    "usage: iqdemod_wide in=cap.iq rate=2048000 tracks=S(1..64) bins=N frames=F modes=<m,...> [gains=<L,...>] "
    "out=pcm_%d.s16 [blocks=K] [lag=0|1] [minstate=1|2] [tracklog=file] [squelch=dBFS,...] [rank=] [ratio_q8=] "
    "[measlog=file] [margin=] [beta_q16=] [carrier=] [minsum=] [carrier_q8=] [wide=] "
    "[guard=] [bridge=] [minwidth=] [maxdet=] [gate_q8=] [open=] [hold=] [alpha_q8=] [bias=] [edges=a,b,c]\n"
    "  (not with offsets=, survey=, scan=, agc=, rxgain=, a fractional rate or format=s8|s16; the capture's whole table\n"
    "  blocks of bins x frames samples are run, a trailing part that does not fill one is dropped and counted;\n"
    "  modes=auto: every channel starts as fm, and the mode chosen from a track's measured hints - carrier am,\n"
    "  narrow fm, wide wbfm - is in force from the call AFTER the one that first sees the track active: a lag of\n"
    "  one call)\n";

// The first thing wrong with the arguments as a whole, as the text to print; empty: nothing.  Fills in what follows from
// them: the decimation P / Q of a bare rate=, and the sample format.
std::string refusal(Options &o)
{
  if (!o.mGiven && o.rate > 0) {   // rate / 256000 = P / Q in lowest terms
    const double r8 = o.rate / 32000.0;
    if (r8 != floor(r8) || r8 < 16 || r8 > 512)
      return "iqdemod_wide: rate must be 256000 P / Q with Q = 1, 2, 4 or 8 and 2 <= P / Q <= 64 (or give decimation=P/Q)\n";
    o.m = (uint32_t)r8;
    o.den = 8;
    while (o.den > 1 && o.m % 2 == 0) {
      o.m /= 2;
      o.den /= 2;
    }
  }
  if (o.format != "u8" && o.format != "s8" && o.format != "s16") return "iqdemod_wide: format must be u8, s8 or s16\n";
  o.sampleFormat = o.format == "s16" ? IQD_WIDE_S16 : o.format == "s8" ? IQD_WIDE_S8 : IQD_WIDE_U8;
  const bool surveying = !o.survey.empty(), scanning = !o.scan.empty(), fractional = o.den > 1, isSigned = o.sampleFormat != IQD_WIDE_U8;
  if (isSigned && (surveying || scanning || fractional))
    return say("iqdemod_wide: format=%s cannot be combined with %s: not built for signed captures yet\n", o.format.c_str(),
               surveying ? "survey=" : scanning ? "scan=" : "a fractional rate");
  bool gainFollowing = !o.rxgain.empty();
  for (const std::string &t : o.agc) {
    if (t != "off" && t != "lowpass" && t != "harris") return "iqdemod_wide: agc must be off, lowpass or harris\n";
    gainFollowing = gainFollowing || t != "off";
  }
  if (gainFollowing && (scanning || fractional || isSigned))
    return say("iqdemod_wide: agc= / rxgain= cannot be combined with %s: channels that follow their gain are not built for it yet\n",
               scanning ? "scan=" : fractional ? "a fractional rate" : "format=s8|s16");
  if (!o.tracks && (o.autoModes || !o.measlog.empty())) return "iqdemod_wide: modes=auto and measlog= need tracks=\n";
  if (o.tracks) {
    if (scanning || gainFollowing || fractional || isSigned)
      return say("iqdemod_wide: tracks= cannot be combined with %s: channels that follow tracks are not built for it yet\n",
                 scanning ? "scan=" : gainFollowing ? "agc= / rxgain=" : fractional ? "a fractional rate" : "format=s8|s16");
    if (o.in.empty() || o.out.empty() || o.modes.empty() || o.gains.empty() || o.m < 2 || o.rate <= 0 || !o.blocks || o.tracks > 64 ||
        !o.bins || !o.frames || o.lag > 1 || o.minstate < 1 || o.minstate > 2 || !o.offsets.empty() || surveying)
      return TRACKS_USAGE;
    const size_t wideBlock = (size_t)2 * o.bins * o.frames;   // capture bytes of one table block; / decimation: its row bytes
    if (wideBlock % o.m != 0 || wideBlock / o.m % 64 != 0) return "iqdemod_wide: tracks= needs 2 bins frames / decimation to be a multiple of 64\n";
    if (!trackEngineBlock(o))
      return "iqdemod_wide: tracks= needs 2 bins frames / decimation (or blocks= of them) to be a multiple of 256, at most 32768\n";
    return "";
  }
  // (iqd_channelizer_survey refuses while a channel follows its scanner)
  if (surveying && scanning) return "iqdemod_wide: survey= cannot be combined with scan=: a survey is refused while a channel follows its scanner\n";
  const bool surveyOk = !surveying || (o.survey.size() == 3 && o.survey[2] >= 1 && o.survey[2] <= 4096 && o.surveyshift <= 8 && !o.surveylog.empty());
  const bool demodOk = !o.offsets.empty() ? !o.out.empty() && !o.modes.empty() : surveying;
  if (o.in.empty() || !demodOk || !surveyOk || o.m < 2 || o.den < 1 || o.rate <= 0 || o.gains.empty() || !o.blocks || o.scan.size() % 3 != 0)
    return USAGE;
  for (uint32_t p = 0; surveying && p < (uint32_t)o.survey[2]; p++)
    if (fabs(o.survey[0] + p * o.survey[1]) >= o.rate / 2)
      return say("iqdemod_wide: survey offset %.0f Hz outside +-rate/2\n", o.survey[0] + p * o.survey[1]);
  for (double off : o.offsets)
    if (fabs(off) >= o.rate / 2) return say("iqdemod_wide: offset %.0f Hz outside +-rate/2\n", off);
  return "";
}

// ---- what both runners do ------------------------------------------------------------------------------------------------------
bool openSinks(Files &files, const std::string &pattern, uint32_t n, std::vector<FILE *> &sinks)
{
  for (uint32_t c = 0; c < n; c++) {
    sinks.push_back(files.open(channelName(pattern, c), "wb", Files::Named));
    if (!sinks.back()) return false;
  }
  return true;
}

// every channel's mode, the rotation of all, and the squelch of each where squelch= was given
int setupChannels(iqd_t *e, const Options &o, uint32_t n, int rotation)
{
  int rc = IQD_OK;
  for (uint32_t c = 0; c < n && rc == IQD_OK; c++) rc = iqd_set_mode(e, c, 1, (int)Options::of(o.modes, c));
  if (rc == IQD_OK && n) rc = iqd_set_rotation(e, 0, n, rotation);
  for (uint32_t c = 0; c < n && rc == IQD_OK && !o.squelch.empty(); c++) rc = iqd_set_squelch(e, c, 1, (int32_t)Options::of(o.squelch, c));
  return rc;
}

// count[c] samples of every channel's row (stride samples apart) to its sink
void writePcm(const std::vector<FILE *> &sinks, const int16_t *pcm, size_t stride, const uint32_t *count, int &status)
{
  for (size_t c = 0; c < sinks.size(); c++)
    if (fwrite(pcm + c * stride, 2, count[c], sinks[c]) != count[c]) {
      fprintf(stderr, "iqdemod_wide: write failed\n");
      status = 1;
    }
}

// ---- tracks= -----------------------------------------------------------------------------------------------------------------
// the tool's copy of the followers' carries, for the log: what a channel is cut with before the call's own table applies
struct Carry {
  std::vector<uint32_t> live, inc;
};

void writeTrackLog(FILE *f, const Options &o, const iqd_track_slot *slots, uint32_t nb, uint64_t blockNo, Carry &carry)
{
  const uint32_t n = o.tracks;
  auto decide = [&](uint32_t b, uint32_t c, uint32_t &live, uint32_t &inc) {
    const iqd_track_slot &q = slots[(size_t)b * n + c];
    live = q.state >= o.minstate ? 1u : 0u;
    inc = live ? q.phase_inc : 0u;
  };
  for (uint32_t b = 0; b < nb; b++)
    for (uint32_t c = 0; c < n; c++) {
      uint32_t live = carry.live[c], inc = carry.inc[c];
      if (b >= o.lag) decide(b - o.lag, c, live, inc);
      fprintf(f, "%llu %u %u 0x%08x %lld\n", (unsigned long long)(blockNo + b), c, live, inc, hzOf(inc, o.rate));
    }
  for (uint32_t c = 0; c < n; c++) decide(nb - 1, c, carry.live[c], carry.inc[c]);
}

void writeMeasLog(FILE *f, const iqd_track_measure *meas, uint32_t nb, uint32_t n, uint64_t blockNo)
{
  for (uint32_t b = 0; b < nb; b++)
    for (uint32_t c = 0; c < n; c++) {
      const iqd_track_measure &q = meas[(size_t)b * n + c];
      if (q.track_id)
        fprintf(f, "m %llu %u %u %u %u %u %u %llu\n", (unsigned long long)(blockNo + b), c, q.track_id, q.flags, q.hint,
                q.flags & IQD_MEASURE_F_EMPTY ? 0u : q.obw_hi - q.obw_lo + 1u, q.carrier_q8, (unsigned long long)q.sum_excess);
    }
}

// modes=auto, one slot after one call: the track_id of the call's last block in which the slot is active, and the mode that
// most of the blocks in which this id is active hint at (ties go to the lowest hint; no hint at all: fm).  id 0: no such block.
int votedMode(const iqd_track_slot *slots, const iqd_track_measure *meas, uint32_t nb, uint32_t n, uint32_t c, uint32_t &id)
{
  id = 0;
  for (uint32_t b = 0; b < nb; b++)
    if (slots[(size_t)b * n + c].state == IQD_TRACK_ACTIVE) id = slots[(size_t)b * n + c].track_id;
  uint32_t votes[4] = {0, 0, 0, 0};
  for (uint32_t b = 0; b < nb; b++) {
    const iqd_track_slot &q = slots[(size_t)b * n + c];
    if (q.state == IQD_TRACK_ACTIVE && q.track_id == id) votes[meas[(size_t)b * n + c].hint & 3]++;
  }
  uint32_t hint = IQD_HINT_NONE;
  for (uint32_t h = IQD_HINT_CARRIER; h <= IQD_HINT_WIDE; h++)
    if (votes[h] > (hint ? votes[hint] : 0u)) hint = h;
  return hint == IQD_HINT_CARRIER ? 1 : hint == IQD_HINT_WIDE ? 3 : 2;
}

// spectrum -> detector -> tracker (-> measurements) -> accept_wideband on one stream per call, one synchronise (the downloads)
int runTracks(const Options &o)
{
  const uint32_t n = o.tracks, N = o.bins, F = o.frames, M = o.m, K = o.blocks;
  const size_t wideBlock = (size_t)2 * N * F, bb = wideBlock / M;   // capture bytes of one table block, and its row bytes
  Files files(TOOL);
  std::vector<FILE *> sinks;
  FILE *f = files.open(o.in, "rb", Files::Named), *tlog = nullptr, *mlog = nullptr;
  if (!f || !openSinks(files, o.out, n, sinks)) return 1;
  if (!o.tracklog.empty() && !(tlog = files.open(o.tracklog, "w", Files::Named))) return 1;
  Engine e;
  int rc = createEngine(e, n, trackEngineBlock(o));
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_wide: iqd_create: %s\n", iqd_strerror(rc));
    return 1;
  }
  if (!o.measlog.empty() && !(mlog = files.open(o.measlog, "w", Files::Named))) return 1;
  const bool measuring = o.autoModes || mlog;
  BandArgs band = o.band;
  band.derive(N, n);
  iqd_spectrum_config sc{};
  sc.n_sources = 1;
  sc.n_bins = N;
  iqd_channelizer_config zc{};
  zc.n_sources = 1;
  zc.n_channels = n;
  zc.decimation = M;
  BandChain chain;
  Channelizer z;
  const char *call = "";
  rc = chain.create(e, sc, band, measuring ? BandChain::MEASURE : BandChain::TRACK, &call);
  if (rc == IQD_OK) rc = iqd_channelizer_create(e, &zc, &z.p);
  std::vector<uint32_t> source(n, 0), inc(n, 0);
  std::vector<uint8_t> shift(n);
  std::vector<int32_t> slot(n);
  std::vector<int> current(n);   // the mode every channel has
  for (uint32_t c = 0; c < n; c++) {
    shift[c] = (uint8_t)Options::of(o.gains, c);
    slot[c] = (int32_t)c;
    current[c] = (int)Options::of(o.modes, c);
  }
  if (rc == IQD_OK) rc = iqd_channelizer_set_channels(z, 0, n, source.data(), inc.data(), shift.data());
  if (rc == IQD_OK) rc = iqd_channelizer_follow_tracks(z, 0, n, slot.data());
  if (rc == IQD_OK) rc = setupChannels(e, o, n, 0);
  const size_t callBytes = K * wideBlock, row = K * bb;
  Buffer<uint8_t> outDev;
  Buffer<int16_t> pcmDev;
  Buffer<uint32_t> countDev;
  if (rc == IQD_OK) rc = chain.alloc(band, K, F);
  if (rc == IQD_OK) rc = outDev.alloc(e, n * row);
  if (rc == IQD_OK) rc = pcmDev.alloc(e, n * (row / 64));
  if (rc == IQD_OK) rc = countDev.alloc(e, n);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_wide: setup: %s (%s)\n", iqd_strerror(rc), iqd_last_error(e));
    return 1;
  }
  std::vector<uint8_t> wide(callBytes);
  std::vector<int16_t> pcm((size_t)n * (row / 64));
  std::vector<uint32_t> count(n);
  std::vector<iqd_track_slot> slots((size_t)K * n);
  std::vector<iqd_track_measure> meas(measuring ? (size_t)K * n : 0);
  Carry carry{std::vector<uint32_t>(n, 0), std::vector<uint32_t>(n, 0)};
  std::vector<uint32_t> decided(n, 0);   // modes=auto: the track_id each channel's mode was chosen for
  uint64_t blockNo = 0;
  size_t dropped = 0;
  int status = 0;
  for (;;) {
    const size_t got = fread(wide.data(), 1, callBytes, f);
    const uint32_t nb = (uint32_t)(got / wideBlock);
    dropped += got - nb * wideBlock;
    if (nb == 0) break;
    const size_t pcmRow = nb * bb / 64;
    iqd_track_follow tf{};
    tf.slots_dev = chain.slots;
    tf.n_slots = n;
    tf.n_blocks = nb;
    tf.block_bytes = (uint32_t)bb;
    tf.lag = o.lag;
    tf.min_state = o.minstate;
    int r = chain.queue(wide.data(), nb, F);
    if (r == IQD_OK) r = iqd_channelizer_set_track_table(z, &tf);
    if (r == IQD_OK) r = iqd_accept_wideband_device(e, z, 0, chain.wide, nb * wideBlock, outDev, pcmDev, countDev, nullptr, nullptr);
    if (r == IQD_OK) r = iqd_synchronize(e);
    if (r == IQD_OK) r = pcmDev.download(pcm.data(), n * pcmRow);
    if (r == IQD_OK) r = countDev.download(count.data(), n);
    if (r == IQD_OK && (tlog || measuring)) r = chain.slots.download(slots.data(), (size_t)nb * n);
    if (r == IQD_OK && measuring) r = chain.meas.download(meas.data(), (size_t)nb * n);
    if (r != IQD_OK) {
      fprintf(stderr, "iqdemod_wide: tracks: %s (%s)\n", iqd_strerror(r), iqd_last_error(e));
      status = 3;
      break;
    }
    writePcm(sinks, pcm.data(), pcmRow, count.data(), status);
    if (tlog) writeTrackLog(tlog, o, slots.data(), nb, blockNo, carry);
    if (mlog) writeMeasLog(mlog, meas.data(), nb, n, blockNo);
    for (uint32_t c = 0; o.autoModes && c < n && status == 0; c++) {
      uint32_t id = 0;
      const int mode = votedMode(slots.data(), meas.data(), nb, n, c, id);
      if (id == 0 || id == decided[c]) continue;
      const int r2 = mode == current[c] ? IQD_OK : iqd_set_mode(e, c, 1, mode);   // (a channel that has the mode is left alone)
      current[c] = mode;
      if (r2 != IQD_OK) {
        fprintf(stderr, "iqdemod_wide: iqd_set_mode: %s (%s)\n", iqd_strerror(r2), iqd_last_error(e));
        status = 3;
        break;
      }
      decided[c] = id;
      if (mlog) fprintf(mlog, "mode %llu %u %u %d\n", (unsigned long long)blockNo, c, id, mode);
    }
    if (status == 3) break;
    blockNo += nb;
    if (got < callBytes) break;
  }
  if (dropped) fprintf(stderr, "iqdemod_wide: %zu trailing bytes do not fill a table block: dropped\n", dropped);
  return status;
}

// ---- fixed, scanning and surveyed channels -------------------------------------------------------------------------------------
struct ChannelRun {
  const Options &o;
  iqd_t *e = nullptr;
  iqd_channelizer_t *z = nullptr;
  const uint32_t n, nPts;             // channels (0: survey only) and survey points
  const size_t rail;                  // bytes per rail
  FILE *slog = nullptr, *flog = nullptr, *glog = nullptr;
  std::vector<FILE *> sinks;
  std::vector<uint32_t> inc, svInc, svMag, count, gtrace;
  std::vector<uint8_t> shift, follows, followsGain, svRows, open;
  std::vector<double> svOff;
  std::vector<uint64_t> cut, trace;   // cut: the frequency each channel's next block is cut at
  std::vector<int16_t> pcm;
  uint64_t blockNo = 0;
  int status = 0;

  explicit ChannelRun(const Options &opt)
      : o(opt), n((uint32_t)opt.offsets.size()), nPts(opt.survey.empty() ? 0 : (uint32_t)opt.survey[2]), rail(opt.format == "s16" ? 2 : 1)
  {
  }

  // the channelizer's channels and survey points, the engine's channels, and who follows a scanner or a gain
  int setup()
  {
    std::vector<uint32_t> source(n, 0);
    std::vector<uint8_t> svShift(nPts, (uint8_t)o.surveyshift);
    for (uint32_t p = 0; p < nPts; p++) {
      svOff.push_back(o.survey[0] + p * o.survey[1]);
      svInc.push_back(incOf(svOff[p], o.rate));
    }
    for (uint32_t c = 0; c < n; c++) {
      inc.push_back(incOf(o.offsets[c], o.rate));
      shift.push_back((uint8_t)Options::of(o.gains, c));
    }
    int rc = IQD_OK;
    if (n) rc = iqd_channelizer_set_channels(z, 0, n, source.data(), inc.data(), shift.data());
    if (rc == IQD_OK && nPts) rc = iqd_channelizer_set_survey(z, nPts, svInc.data(), svShift.data());
    if (rc == IQD_OK) rc = setupChannels(e, o, n, o.rotation);
    // scanning channels: their scanners and the channelizer's following flags
    follows.assign(n, 0);
    if (rc == IQD_OK) rc = iqd_channelizer_set_source_frequency(z, 0, 1, &o.centre);
    for (uint32_t c = 0; c < n && rc == IQD_OK && !o.scan.empty(); c++) {
      const uint64_t *g = &o.scan[3 * (c % (o.scan.size() / 3))];
      if (!g[0] && !g[1] && !g[2]) continue;
      rc = iqd_scanner_set_parameters(e, c, 1, g[0], g[1], g[2]);
      if (rc == IQD_OK) rc = iqd_scanner_start(e, c, 1, 1);
      if (rc == IQD_OK) rc = iqd_channelizer_follow_scanner(z, c, 1, 1);
      follows[c] = 1;
    }
    // channels that follow their gain: a running AGC, or a gain in dB of their own
    followsGain.assign(n, 0);
    for (uint32_t c = 0; c < n && rc == IQD_OK; c++) {
      const std::string t = o.agc.empty() ? "off" : Options::of(o.agc, c);
      if (!o.rxgain.empty()) rc = iqd_set_rx_gain_db(e, c, 1, (uint32_t)Options::of(o.rxgain, c));
      if (rc == IQD_OK && t != "off") rc = iqd_agc_set_type(e, c, 1, t == "harris" ? IQD_AGC_HARRIS : IQD_AGC_LOWPASS);
      if (rc == IQD_OK && t != "off") rc = iqd_agc_enable(e, c, 1, 1);
      followsGain[c] = t != "off" || !o.rxgain.empty();
      if (rc == IQD_OK && followsGain[c]) rc = iqd_channelizer_follow_gain(z, c, 1, 1);
    }
    if (rc == IQD_OK && glog) rc = iqd_set_gain_trace(e, 1);
    // the frequency each channel's first block is cut at: the scanner's (its start() jump applied), or the fixed one
    cut.assign(n, 0);
    if (rc == IQD_OK && flog) rc = iqd_set_gain_trace(e, 1);
    for (uint32_t c = 0; c < n && rc == IQD_OK && flog; c++) {
      if (follows[c]) rc = iqd_scanner_get(e, c, &cut[c], nullptr, nullptr);
      else cut[c] = (uint64_t)((int64_t)o.centre + llround(o.offsets[c]) - 64000 * (int64_t)o.rotation);
    }
    return rc;
  }

  // before the run (a survey reads the state the accept starts from): nblk blocks' magnitudes at every point, to surveylog
  int survey(const uint8_t *p, size_t bytes, size_t nblk)
  {
    const size_t bb = bytes / o.m * o.den / nblk;   // row bytes per block
    if (bb % (o.den > 1 ? 256 : 64) != 0) {
      fprintf(stderr, "iqdemod_wide: the short block of %zu row bytes is not surveyed\n", bb);
      return IQD_OK;
    }
    const int r = iqd_channelizer_survey(z, p, bytes, (uint32_t)bb, svMag.data());
    for (size_t b = 0; r == IQD_OK && b < nblk; b++)
      for (uint32_t q = 0; q < nPts; q++) {
        const uint32_t mg = svMag[b * nPts + q];
        fprintf(slog, "%llu %lld %u %d\n", (unsigned long long)(blockNo + b), (long long)llround(svOff[q]), mg, (int)iqd_magnitude_dbfs(mg));
      }
    return r;
  }

  void writeLogs(size_t nblk)
  {
    for (size_t b = 0; flog && b < nblk; b++)
      for (uint32_t c = 0; c < n; c++) {
        fprintf(flog, "%llu %u %llu %u\n", (unsigned long long)(blockNo + b), c, (unsigned long long)cut[c], (unsigned)open[(size_t)c * nblk + b]);
        if (follows[c]) cut[c] = trace[(size_t)c * nblk + b];   // the frequency after this block's scanner step
      }
    for (size_t b = 0; glog && b < nblk; b++)
      for (uint32_t c = 0; c < n; c++) {
        const uint32_t g = gtrace[(size_t)c * nblk + b];
        fprintf(glog, "%llu %u %u\n", (unsigned long long)(blockNo + b), c,
                followsGain[c] ? (g < IQD_GAIN_FOLLOW_MAX ? g : (uint32_t)IQD_GAIN_FOLLOW_MAX) : 6u * shift[c]);
      }
  }

  // one accept of `bytes` (whole engine blocks, or ONE short block: include/iqdemod.h), its PCM and its log lines out
  bool feed(const uint8_t *p, size_t bytes, size_t block)
  {
    const size_t nblk = bytes % block == 0 ? bytes / block : 1;
    int r = nPts ? survey(p, bytes, nblk) : IQD_OK;
    // survey only: nothing is demodulated, but the stream moves on - the one channel at offset 0 is run (its row comes
    // back to the host and is dropped: 1 / M of the capture's bytes, the price of advancing the history over the C ABI)
    const char *what = r == IQD_OK && !n ? "survey" : "accept";
    if (r == IQD_OK && !n) r = iqd_channelizer_run(z, p, bytes, svRows.data());
    if (r == IQD_OK && n) r = iqd_accept_wideband(e, z, 0, p, bytes, pcm.data(), count.data(), nullptr, flog ? open.data() : nullptr);
    if (r == IQD_OK && n && flog) {
      trace.resize((size_t)n * nblk);
      r = iqd_get_frequency_trace(e, 0, n, trace.data(), nblk);
    }
    if (r == IQD_OK && n && glog) {
      gtrace.resize((size_t)n * nblk);
      r = iqd_get_gain_trace(e, 0, n, gtrace.data(), nblk);
    }
    if (r != IQD_OK) {
      fprintf(stderr, "iqdemod_wide: %s: %s (%s)\n", what, iqd_strerror(r), iqd_last_error(e));
      status = 3;
      return false;
    }
    if (n) writePcm(sinks, pcm.data(), bytes / o.m / rail * o.den / 64, count.data(), status);
    if (n) writeLogs(nblk);
    blockNo += nblk;
    return true;
  }
};

int runChannels(const Options &o)
{
  ChannelRun run(o);
  const uint32_t n = run.n, m = o.m, den = o.den;
  Files files(TOOL);
  FILE *f = files.open(o.in, "rb", Files::Named);
  if (!f || !openSinks(files, o.out, n, run.sinks)) return 1;
  if (run.nPts && !(run.slog = files.open(o.surveylog, "w", Files::Named))) return 1;
  if (!o.freqlog.empty() && !(run.flog = files.open(o.freqlog, "w", Files::Named))) return 1;
  if (!o.gainlog.empty() && !(run.glog = files.open(o.gainlog, "w", Files::Named))) return 1;
  Engine e;
  int rc = createEngine(e, n ? n : 1);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_wide: iqd_create: %s\n", iqd_strerror(rc));
    return 1;
  }
  iqd_channelizer_config zc{};
  zc.n_sources = 1;
  zc.n_channels = n ? n : 1;   // (survey only: one channel at offset 0 carries the stream's history along)
  zc.decimation = m;
  zc.decimation_den = den;
  zc.sample_format = o.sampleFormat;
  Channelizer z;
  rc = iqd_channelizer_create(e, &zc, &z.p);
  run.e = e;
  run.z = z;
  if (rc == IQD_OK) rc = run.setup();
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_wide: setup: %s (%s)\n", iqd_strerror(rc), iqd_last_error(e));
    return 1;
  }
  // (wide bytes per engine block: 32768 m / den = 64 m (512 / den), whole calls of the channelizer)
  // (rail bytes per rail: a signed 16-bit capture has twice the bytes per block; den is 1 there)
  const size_t block = 32768 / den * (size_t)m * run.rail, call = o.blocks * block, unit = 64 * (size_t)m * run.rail;
  std::vector<uint8_t> wide(call);
  run.pcm.resize((size_t)n * call / m / run.rail * den / 64);
  run.svMag.resize((size_t)o.blocks * run.nPts);
  run.svRows.resize(n ? 0 : call / m * den);
  run.count.resize(n);
  run.open.resize((size_t)n * o.blocks);
  for (;;) {
    size_t got = fread(wide.data(), 1, call, f);
    got -= got % unit;
    if (got == 0) break;
    // a capture that ends inside a call: its whole blocks first, then the rest as one short block
    const size_t whole = got / block * block, rest = got - whole;
    if (whole && !run.feed(wide.data(), whole, block)) break;
    if (rest && !run.feed(wide.data() + whole, rest, block)) break;
    if (got < call) break;
  }
  return run.status;
}

}  // namespace

int main(int argc, char **argv)
{
  Options o;
  if (!parse(argc, argv, o.keys(), TOOL)) return 1;
  const std::string why = refusal(o);
  if (!why.empty()) {
    fputs(why.c_str(), stderr);
    return 1;
  }
  return o.tracks ? runTracks(o) : runChannels(o);
}
