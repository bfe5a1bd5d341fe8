// iqdemod_tones — which tone is in a channel's PCM, straight over the C ABI (include/iqdemod_tones.h: iqd_tones_*): S16_LE
// PCM from stdin, or many channels at once from files, through one tone bank; one text line per frame that opens or closes
// a tone.  Chains behind a demodulator:  iqdemod_file 2 < cap.iq | iqdemod_tones set=ctcss
//
//   iqdemod_tones set=ctcss|dtmf | tones=f1,f2,... [rate=8000] [frame=4096] [ratio_q8=512] [energy_q8=0] [minpower=0]
//                 [open=2] [hold=1] [channels=N in=pcm_%d.s16] [log=tones.txt] [chunk=samples]
//
//   set       ctcss: the 50 standard sub-audible tones, frame=4096 ratio_q8=512 open=2 hold=1 unless given (at 2048 the
//             67.0 / 69.3 Hz pair is too close); dtmf: the four row and four column tones, frame=256 ratio_q8=256 open=1
//             hold=0 unless given (a digit shows as best and second: its row and its column)
//   tones     the tones in Hz, decimals allowed (up to 64)
//   rate      the PCM's sample rate in Hz (default 8000)
//   channels  N streams through one tone bank: in= is a file name pattern with one %d (the channel).  Left out: one
//             stream from stdin.
//   log       where the lines go (default: stdout).  A line:
//               ch C frame K t SECONDS OPENED|CLOSED|SWITCHED tone INDEX HZ p_best P p_second P energy E
//             frame K counts the channel's frames from 0, SECONDS is the frame's end; the tone is the one that opened, or
//             for CLOSED the one that closed
//   chunk     samples per channel and call (default 65536); frames straddle calls, so the output does not depend on it
// Exit status 0, 1 (no device / bad arguments / I/O), 3 (a call was rejected).
#include <math.h>

#include "iqd_tool_chain.h"
#include "iqdemod_tones.h"

using namespace iqdtool;

static const char *const USAGE =
    "usage: iqdemod_tones set=ctcss|dtmf | tones=f1,f2,... [rate=8000] [frame=4096] [ratio_q8=512] [energy_q8=0] [minpower=0] "
    "[open=2] [hold=1] [channels=N in=pcm_%d.s16] [log=tones.txt] [chunk=samples]\n";

int main(int argc, char **argv)
{
  const char *const TOOL = "iqdemod_tones";
  std::string set, list, in, log;
  uint32_t rate = 8000, channels = 0;
  size_t chunk = 65536;
  iqd_tones_config cfg{};
  bool frameGiven = false, ratioGiven = false, openGiven = false, holdGiven = false;
  const std::vector<Row> keys = {text("set=", set), text("tones=", list), u32("rate=", rate), u32("frame=", cfg.frame_len, &frameGiven),
                                 u32("ratio_q8=", cfg.ratio_q8, &ratioGiven), u32("energy_q8=", cfg.energy_q8),
                                 viaStrtoull("minpower=", cfg.min_power), u32("open=", cfg.open, &openGiven), u32("hold=", cfg.hold, &holdGiven),
                                 u32("channels=", channels), text("in=", in), text("log=", log), viaStrtoull("chunk=", chunk)};
  if (!parse(argc, argv, keys, TOOL)) return 1;
  const bool fromFiles = channels != 0;
  std::vector<uint32_t> mhz;
  if (set == "ctcss" && list.empty()) {
    mhz.resize(50);
    iqd_tones_ctcss(mhz.data());
  } else if (set == "dtmf" && list.empty()) {
    mhz.resize(8);
    iqd_tones_dtmf(mhz.data());
  } else if (set.empty()) {
    for (double hz : doubleList(list.c_str())) mhz.push_back((uint32_t)llround(hz * 1000.0));
  }
  if (mhz.empty() || mhz.size() > 64 || chunk == 0 || chunk > 0x7fffffffu || fromFiles != !in.empty()) {
    fputs(USAGE, stderr);
    return 1;
  }
  const bool dtmf = set == "dtmf";
  if (!frameGiven) cfg.frame_len = dtmf ? 256 : 4096;
  if (!ratioGiven) cfg.ratio_q8 = dtmf ? 256 : 512;
  if (!openGiven) cfg.open = dtmf ? 1 : 2;
  if (!holdGiven) cfg.hold = dtmf ? 0 : 1;
  std::vector<uint32_t> inc(mhz.size());
  for (size_t t = 0; t < mhz.size(); t++)
    if (iqd_tones_phase_inc(mhz[t], rate, &inc[t]) != IQD_OK) {
      fprintf(stderr, "iqdemod_tones: a tone of %.3f Hz needs a rate above %.3f Hz (rate=%u)\n", mhz[t] / 1000.0, mhz[t] / 500.0, rate);
      return 1;
    }
  const uint32_t n = fromFiles ? channels : 1;

  Files files(TOOL);
  PcmInput input;
  if (!input.open(files, in, channels, chunk, [](uint32_t) { return true; })) return 1;
  FILE *out = log.empty() ? stdout : files.open(log, "w", Files::Named);
  if (!out) return 1;

  Engine e;
  if (!createPcmEngine(e, TOOL)) return 1;
  cfg.abi_version = IQD_TONES_ABI_VERSION;
  cfg.n_channels = n;
  cfg.n_tones = (uint32_t)inc.size();
  cfg.phase_inc = inc.data();
  Handle<iqd_tones_t, iqd_tones_destroy> bank;
  int rc = iqd_tones_create(e, &cfg, &bank.p);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_tones: iqd_tones_create: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
    return 1;
  }

  const size_t maxFrames = iqd_tones_max_frames(bank, chunk);
  std::vector<uint32_t> done(n);
  std::vector<iqd_tones_frame> frames((size_t)n * (maxFrames ? maxFrames : 1));
  std::vector<uint64_t> seen(n, 0);      // frames of the channel so far
  std::vector<int32_t> tone(n, -1);      // the tone in force
  int status = 0;
  for (size_t got; status == 0 && input.read(got);) {
    const size_t F = iqd_tones_max_frames(bank, got);
    rc = iqd_tones_run(e, bank, input.pcm.data(), chunk, input.count.data(), got, done.data(), frames.data(), nullptr);
    if (rc != IQD_OK) {
      fprintf(stderr, "iqdemod_tones: iqd_tones_run: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
      status = 3;
      break;
    }
    for (uint32_t c = 0; c < n; c++)
      for (uint32_t k = 0; k < done[c]; k++, seen[c]++) {
        const iqd_tones_frame &r = frames[(size_t)c * F + k];
        if (r.flags) {
          const bool opened = r.flags & IQD_TONES_F_OPENED, closed = r.flags & IQD_TONES_F_CLOSED;
          const int32_t named = opened ? r.tone : tone[c];
          fprintf(out, "ch %u frame %llu t %.3f %s tone %d %.3f p_best %llu p_second %llu energy %llu\n", c, (unsigned long long)seen[c],
                  (double)(seen[c] + 1) * cfg.frame_len / rate, opened && closed ? "SWITCHED" : opened ? "OPENED" : "CLOSED", named,
                  named >= 0 ? mhz[named] / 1000.0 : 0.0, (unsigned long long)r.p_best, (unsigned long long)r.p_second,
                  (unsigned long long)r.energy);
        }
        tone[c] = r.tone;
      }
  }
  return closeOutputs(files, status);
}
