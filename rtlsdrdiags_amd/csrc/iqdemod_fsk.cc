// iqdemod_fsk — the packet frames in a channel's PCM, straight over the C ABI (include/iqdemod_fsk.h: iqd_fsk_*): S16_LE PCM
// from stdin, or many channels at once from files, through one decoder; one text line per HDLC frame with a good FCS.
// Chains behind a demodulator like `rtl_fm | multimon-ng -a AFSK1200`:  iqdemod_file 2 < cap.iq | iqdemod_fsk set=afsk1200
//
//   iqdemod_fsk set=afsk1200 | mark=HZ space=HZ baud=BD [rate=8000] [corr=8] [loop=3] [nrzi=1] [minlen=17] [maxlen=512]
//               [channels=N in=pcm_%d.s16] [log=frames.txt] [bits=bits_%d.txt] [chunk=samples]
//
//   set       afsk1200: Bell 202 as APRS / AX.25 packet uses it - mark=1200 space=2200 baud=1200 corr=8 loop=3 nrzi=1 minlen=17
//             maxlen=512; the arguments given beside it replace its values
//   mark, space, baud   the two tones in Hz and the bit rate, decimals allowed
//   rate      the PCM's sample rate in Hz (default 8000)
//   corr, loop, nrzi, minlen, maxlen   corr_len, loop_shift, IQD_FSK_NRZI (0 or 1), min_len, max_len of iqd_fsk_config
//   channels  N streams through one decoder: in= is a file name pattern with one %d (the channel).  Left out: one stream
//             from stdin.
//   log       where the lines go (default: stdout).  A line:
//               ch C end SAMPLE t SECONDS len BYTES [SRC>DST[,PATH] ]HEX
//             SAMPLE is the channel's sample at which the closing flag ended, SECONDS the same as time, BYTES the payload
//             without the FCS, HEX the payload; SRC>DST[,PATH] stands where the first bytes parse as AX.25 addresses
//   bits      a file per channel (a pattern with one %d; without channels= a plain name): every bit after NRZI as 0 or 1
//   chunk     samples per channel and call (default 65536); the state is carried, so the output does not depend on it
// Exit status 0, 1 (no device / bad arguments / I/O), 3 (a call was rejected).
#include <math.h>

#include "iqd_tool_chain.h"
#include "iqdemod_fsk.h"

using namespace iqdtool;

static const char *const USAGE =
    "usage: iqdemod_fsk set=afsk1200 | mark=HZ space=HZ baud=BD [rate=8000] [corr=8] [loop=3] [nrzi=1] [minlen=17] [maxlen=512] "
    "[channels=N in=pcm_%d.s16] [log=frames.txt] [bits=bits_%d.txt] [chunk=samples]\n";

// "SRC>DST[,PATH] " where the payload starts with AX.25 addresses (seven bytes each: six characters shifted left by one, then
// the SSID byte whose lowest bit ends the list; destination first, then the source, then up to eight repeaters), else ""
static std::string ax25Addresses(const uint8_t *p, size_t len)
{
  std::vector<std::string> names;
  for (size_t at = 0; at + 7 <= len && names.size() < 10; at += 7) {
    std::string s;
    for (int i = 0; i < 6; i++) {
      const uint8_t b = p[at + i];
      const char ch = (char)(b >> 1);
      if ((b & 1) || !((ch >= 'A' && ch <= 'Z') || (ch >= '0' && ch <= '9') || ch == ' ')) return "";
      s += ch;
    }
    while (!s.empty() && s.back() == ' ') s.pop_back();
    if (s.empty() || s.find(' ') != std::string::npos) return "";
    const unsigned ssid = (p[at + 6] >> 1) & 15u;
    if (ssid) s += "-" + std::to_string(ssid);
    names.push_back(s);
    if (p[at + 6] & 1) {
      if (names.size() < 2) return "";
      std::string out = names[1] + ">" + names[0];
      for (size_t i = 2; i < names.size(); i++) out += "," + names[i];
      return out + " ";
    }
  }
  return "";
}

int main(int argc, char **argv)
{
  const char *const TOOL = "iqdemod_fsk";
  std::string set, in, log, bitsName;
  double mark = 0, space = 0, baud = 0;
  uint32_t rate = 8000, channels = 0, corr = 8, loop = 3, nrzi = 1, minlen = 17, maxlen = 512;
  size_t chunk = 65536;
  const std::vector<Row> keys = {text("set=", set), real("mark=", mark), real("space=", space), real("baud=", baud), u32("rate=", rate),
                                 u32("corr=", corr), u32("loop=", loop), u32("nrzi=", nrzi), u32("minlen=", minlen), u32("maxlen=", maxlen),
                                 u32("channels=", channels), text("in=", in), text("log=", log), text("bits=", bitsName),
                                 viaStrtoull("chunk=", chunk)};
  if (!parse(argc, argv, keys, TOOL)) return 1;
  const bool fromFiles = channels != 0;
  if (set == "afsk1200") {
    if (mark == 0) mark = 1200;
    if (space == 0) space = 2200;
    if (baud == 0) baud = 1200;
  }
  if ((!set.empty() && set != "afsk1200") || mark <= 0 || space <= 0 || baud <= 0 || nrzi > 1 || chunk == 0 || chunk > 0x7fffffffu ||
      fromFiles != !in.empty()) {
    fputs(USAGE, stderr);
    return 1;
  }
  iqd_fsk_config cfg{};
  const double hz[3] = {mark, space, baud};
  uint32_t *const inc[3] = {&cfg.mark_inc, &cfg.space_inc, &cfg.baud_inc};
  for (int i = 0; i < 3; i++)
    if (iqd_fsk_phase_inc((uint64_t)llround(hz[i] * 1000.0), rate, inc[i]) != IQD_OK) {
      fprintf(stderr, "iqdemod_fsk: %.3f Hz needs a rate above %.3f Hz (rate=%u)\n", hz[i], 2.0 * hz[i], rate);
      return 1;
    }
  const uint32_t n = fromFiles ? channels : 1;

  Files files(TOOL);
  std::vector<FILE *> fbits(n, nullptr);
  PcmInput input;
  if (!input.open(files, in, channels, chunk, [&](uint32_t c) {
        return bitsName.empty() || (fbits[c] = files.open(fromFiles ? channelName(bitsName, c) : bitsName, "w", Files::Named));
      }))
    return 1;
  FILE *out = log.empty() ? stdout : files.open(log, "w", Files::Named);
  if (!out) return 1;

  Engine e;
  if (!createPcmEngine(e, TOOL)) return 1;
  cfg.abi_version = IQD_FSK_ABI_VERSION;
  cfg.n_channels = n;
  cfg.corr_len = corr;
  cfg.loop_shift = loop;
  cfg.flags = nrzi ? IQD_FSK_NRZI : 0;
  cfg.min_len = minlen;
  cfg.max_len = maxlen;
  Handle<iqd_fsk_t, iqd_fsk_destroy> modem;
  int rc = iqd_fsk_create(e, &cfg, &modem.p);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_fsk: iqd_fsk_create: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
    return 1;
  }

  std::vector<uint32_t> nBits(n), nFrames(n);
  std::vector<uint32_t> bits((size_t)n * iqd_fsk_max_bit_words(modem, chunk));
  std::vector<iqd_fsk_frame> frames((size_t)n * iqd_fsk_max_frames(modem, chunk));
  std::vector<uint8_t> bytes((size_t)n * iqd_fsk_max_bytes(modem, chunk));
  int status = 0;
  for (size_t got; status == 0 && input.read(got);) {
    const size_t F = iqd_fsk_max_frames(modem, got), Bw = iqd_fsk_max_bit_words(modem, got), Bc = iqd_fsk_max_bytes(modem, got);
    rc = iqd_fsk_run(e, modem, input.pcm.data(), chunk, input.count.data(), got, nBits.data(), bitsName.empty() ? nullptr : bits.data(), nFrames.data(),
                     frames.data(), bytes.data());
    if (rc != IQD_OK) {
      fprintf(stderr, "iqdemod_fsk: iqd_fsk_run: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
      status = 3;
      break;
    }
    for (uint32_t c = 0; c < n; c++) {
      for (uint32_t i = 0; fbits[c] && i < nBits[c]; i++) fputc('0' + ((bits[(size_t)c * Bw + i / 32] >> (i % 32)) & 1u), fbits[c]);
      for (uint32_t k = 0; k < nFrames[c]; k++) {
        const iqd_fsk_frame &r = frames[(size_t)c * F + k];
        const uint8_t *p = bytes.data() + (size_t)c * Bc + r.offset;
        fprintf(out, "ch %u end %llu t %.4f len %u %s", c, (unsigned long long)r.end_sample, (double)r.end_sample / rate, r.len,
                ax25Addresses(p, r.len).c_str());
        for (uint32_t i = 0; i < r.len; i++) fprintf(out, "%02x", p[i]);
        fputc('\n', out);
      }
    }
  }
  return closeOutputs(files, status);
}
