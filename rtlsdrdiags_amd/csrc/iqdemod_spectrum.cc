// iqdemod_spectrum — the band spectrum of one wideband capture file, straight over the C ABI (include/iqdemod.h:
// iqd_spectrum_*): what a user looks at before placing survey points or channels.
//
//   iqdemod_spectrum in=cap.iq rate=2048000 bins=1024 frames=250 format=u8|s8 [window=w.txt] out=power.u32 [log=spectrum.txt]
//
//   in       interleaved I/Q, one byte per rail
//   rate     the capture's sample rate in Hz (for the log's offsets only)
//   bins     N: 64, 128, 256, 512, 1024 or 2048
//   frames   F: frames of N samples per block; one spectrum per block
//   format   u8 (offset binary, the default) or s8
//   window   a text file of N int16 values separated by white space or commas; left out: the library's default window
//   out      the API's array, block after block: N little-endian uint32 per block
//   log      one line per block and bin: block, offset in Hz ((k' - N / 2) rate / N), power, dBFS
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
  std::string in, out, log, windowPath, format = "u8";
  double rate = 0.0;
  uint32_t bins = 0, frames = 0;
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
    else {
      fprintf(stderr, "iqdemod_spectrum: unknown argument %s\n", a);
      return 1;
    }
  }
  const bool u8 = format == "u8";
  if (in.empty() || out.empty() || bins == 0 || frames == 0 || frames > (1u << 24) || !(rate > 0.0) || (!u8 && format != "s8")) {
    fprintf(stderr, "usage: iqdemod_spectrum in=cap.iq rate=2048000 bins=1024 frames=250 format=u8|s8 [window=w.txt] "
                    "out=power.u32 [log=spectrum.txt]\n");
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
  if (!fin || !fout || (!log.empty() && !flog)) {
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

  // whole blocks, up to about 16 MiB of capture per call
  const size_t blockBytes = (size_t)2 * bins * frames;
  const size_t perCall = blockBytes >= (16u << 20) ? 1 : (16u << 20) / blockBytes;
  std::vector<uint8_t> buf(perCall * blockBytes);
  std::vector<uint32_t> power(perCall * bins);
  int status = 0;
  uint64_t block = 0;
  size_t dropped = 0;
  for (;;) {
    const size_t got = fread(buf.data(), 1, buf.size(), fin);
    const size_t nb = got / blockBytes;
    dropped = got - nb * blockBytes;
    if (nb) {
      rc = iqd_spectrum_run(s, buf.data(), nb * blockBytes, frames, power.data());
      if (rc != IQD_OK) {
        fprintf(stderr, "iqdemod_spectrum: iqd_spectrum_run: %s: %s\n", iqd_strerror(rc), iqd_last_error(e));
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
      block += nb;
    }
    if (got < buf.size()) break;
  }
  if (dropped) fprintf(stderr, "iqdemod_spectrum: %zu bytes after the last whole block dropped\n", dropped);
  iqd_spectrum_destroy(s);
  iqd_destroy(e);
  fclose(fin);
  if (fclose(fout) != 0) status = status ? status : 1;
  if (flog && fclose(flog) != 0) status = status ? status : 1;
  return status;
}
