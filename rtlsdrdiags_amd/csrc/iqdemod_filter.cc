// iqdemod_filter — the reference's Filters/Int16/decimateAudio.cc generalised, straight over the C ABI (include/iqdemod.h:
// iqd_filter_*): raw samples from stdin through one of the reference's four filter classes to stdout, or many channels
// at once from and to files.  int16 samples (S16_LE) for the two I16 kinds, float32 for the two F32 kinds.
//
//   iqdemod_filter kind=decimate_i16|fir_i16|fir_f32|iir_f32 taps=h.txt [factor=4] [den=a.txt]
//                  [channels=N in=x_%d.raw out=y_%d.raw] [chunk=samples]
//
//   taps      a text file of coefficients separated by white space or commas (the IIR's numerator)
//   den       iir_f32: the denominator without its leading 1
//   factor    decimate_i16: one output per `factor` inputs (default 1)
//   channels  N streams through one filter object: in= and out= are file name patterns with one %d (the channel); every
//             input must hold the same number of samples.  Left out: one stream from stdin to stdout.
//   chunk     samples per channel and call (default 65536); the filter state carries over, so the output does not depend
//             on it
// Exit status 0, 1 (no device / bad arguments / I/O), 3 (a call was rejected).
#include "iqd_tool_chain.h"

using namespace iqdtool;

int main(int argc, char **argv)
{
  const char *const TOOL = "iqdemod_filter";
  std::string kindName, tapsPath, denPath, in, out;
  uint32_t factor = 1, channels = 0;
  size_t chunk = 65536;
  const std::vector<Row> keys = {text("kind=", kindName), text("taps=", tapsPath),  text("den=", denPath), u32("factor=", factor),
                                 u32("channels=", channels), text("in=", in), text("out=", out), viaStrtoull("chunk=", chunk)};
  if (!parse(argc, argv, keys, TOOL)) return 1;
  static const char *const kinds[] = {"decimate_i16", "fir_i16", "fir_f32", "iir_f32"};
  int kind = -1;
  for (int k = 0; k < 4; k++)
    if (kindName == kinds[k]) kind = k;
  const bool fromFiles = channels != 0;
  if (kind < 0 || tapsPath.empty() || chunk == 0 || chunk > 0x7fffffffu || (fromFiles && (in.empty() || out.empty())) ||
      (!fromFiles && (!in.empty() || !out.empty()))) {
    fprintf(stderr, "usage: iqdemod_filter kind=decimate_i16|fir_i16|fir_f32|iir_f32 taps=h.txt [factor=4] [den=a.txt] "
                    "[channels=N in=x_%%d.raw out=y_%%d.raw] [chunk=samples]\n");
    return 1;
  }
  std::vector<float> num, den;
  const auto coefficient = [](const char *tok, float &x) {
    x = strtof(tok, nullptr);
    return true;
  };
  if (!readNumbers(tapsPath, num, coefficient)) {
    fprintf(stderr, "iqdemod_filter: no coefficients in %s\n", tapsPath.c_str());
    return 1;
  }
  if (!denPath.empty() && !readNumbers(denPath, den, coefficient)) {
    fprintf(stderr, "iqdemod_filter: no coefficients in %s\n", denPath.c_str());
    return 1;
  }
  const uint32_t n = fromFiles ? channels : 1;
  const size_t elem = kind <= IQD_FILTER_FIR_I16 ? 2 : 4;

  Files files(TOOL);
  std::vector<FILE *> fin(n, nullptr), fout(n, nullptr);
  for (uint32_t c = 0; c < n; c++) {
    fin[c] = fromFiles ? files.open(channelName(in, c), "rb", Files::Quiet) : stdin;
    fout[c] = fromFiles ? files.open(channelName(out, c), "wb", Files::Quiet) : stdout;
    if (!fin[c] || !fout[c]) {
      fprintf(stderr, "iqdemod_filter: cannot open the files of channel %u\n", c);
      return 1;
    }
  }

  Engine e;
  int rc = createEngine(e, 1);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_filter: iqd_create: %s\n", iqd_strerror(rc));
    return 1;
  }
  Filter f;
  rc = iqd_filter_create(e, kind, num.data(), (uint32_t)num.size(), den.empty() ? nullptr : den.data(), (uint32_t)den.size(),
                         factor, n, &f.p);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_filter: iqd_filter_create: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
    return 1;
  }

  std::vector<uint8_t> xin(n * chunk * elem), yout(n * chunk * elem);
  std::vector<std::vector<uint8_t>> rows(n, std::vector<uint8_t>(chunk * elem));
  int status = 0;
  for (;;) {
    // every channel gives the same number of samples per call: the shortest read decides, and ends the run
    size_t got = chunk;
    for (uint32_t c = 0; c < n; c++) {
      const size_t r = fread(rows[c].data(), elem, chunk, fin[c]);
      if (r < got) got = r;
    }
    if (got == 0) break;
    for (uint32_t c = 0; c < n; c++) memcpy(xin.data() + (size_t)c * got * elem, rows[c].data(), got * elem);
    const size_t n_out = iqd_filter_out_count(f, got);
    rc = iqd_filter_run(f, xin.data(), got, yout.data());
    if (rc != IQD_OK) {
      fprintf(stderr, "iqdemod_filter: iqd_filter_run: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
      status = 3;
      break;
    }
    for (uint32_t c = 0; c < n && status == 0; c++)
      if (n_out && fwrite(yout.data() + (size_t)c * n_out * elem, elem, n_out, fout[c]) != n_out) {
        fprintf(stderr, "iqdemod_filter: write failed on channel %u\n", c);
        status = 1;
      }
    if (status != 0 || got < chunk) break;
  }
  if ((fromFiles ? !files.close() : fflush(stdout) != 0) && status == 0) status = 1;
  return status;
}
