// iqdemod_wide — many channels out of ONE wideband capture, straight over the C ABI (include/iqdemod.h): the one-receiver
// counterpart of iqdemod_multi.  The capture is uint8 interleaved I/Q at decimation x 256 kS/s (an RTL-SDR at 2.048 MS/s
// is decimation=8, one at 2.4 MS/s decimation=75/8); every channel is cut out by the channelizer (iqd_channelizer_*) at its offset from the capture's
// centre and demodulated by one engine channel - one reference IqDataProcessor with its demodulators (Radio.cc:150-181).
// PCM goes out as S16_LE at 8 kS/s (radioApp.cc:103-111), one file per channel.
//
//   iqdemod_wide in=cap.iq [decimation=8] rate=2048000 offsets=<Hz>[,<Hz>...] modes=<m>[,<m>...] [gains=<L>[,<L>...]]
//                out=pcm_%d.s16 [blocks=K] [rotation=<r>] [centre=<Hz>] [scan=<start>,<end>,<step>[,...]]
//                [squelch=<dBFS>[,<dBFS>...]] [freqlog=<file>]
//
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

}  // namespace

int main(int argc, char **argv)
{
  std::string in, out, freqlog;
  uint32_t m = 0, den = 1, blocks = 4;
  bool m_given = false;
  double rate = 0;
  int rotation = 1;
  uint64_t centre = 0;
  std::vector<double> offsets, modes, gains{0}, squelch;
  std::vector<uint64_t> scan;
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
    else if (!strncmp(a, "modes=", 6)) modes = numList(a + 6);
    else if (!strncmp(a, "gains=", 6)) gains = numList(a + 6);
    else if (!strncmp(a, "blocks=", 7)) blocks = (uint32_t)atoi(a + 7);
    else if (!strncmp(a, "rotation=", 9)) rotation = atoi(a + 9);
    else if (!strncmp(a, "centre=", 7)) centre = strtoull(a + 7, nullptr, 10);
    else if (!strncmp(a, "scan=", 5)) scan = u64List(a + 5);
    else if (!strncmp(a, "squelch=", 8)) squelch = numList(a + 8);
    else if (!strncmp(a, "freqlog=", 8)) freqlog = a + 8;
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
  if (in.empty() || out.empty() || m < 2 || den < 1 || rate <= 0 || offsets.empty() || modes.empty() || gains.empty() || !blocks ||
      scan.size() % 3 != 0) {
    fprintf(stderr, "usage: iqdemod_wide in=cap.iq [decimation=8|75/8] rate=2048000 offsets=<Hz,...> modes=<m,...> "
                    "[gains=<L,...>] out=pcm_%%d.s16 [blocks=K] [rotation=r] [centre=Hz] [scan=start,end,step,...] "
                    "[squelch=dBFS,...] [freqlog=file]\n");
    return 1;
  }
  const uint32_t n = (uint32_t)offsets.size();
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
  FILE *flog = nullptr;
  if (!freqlog.empty() && !(flog = fopen(freqlog.c_str(), "w"))) {
    fprintf(stderr, "iqdemod_wide: cannot create %s\n", freqlog.c_str());
    return 1;
  }

  iqd_config cfg{};
  cfg.abi_version = IQD_ABI_VERSION;
  cfg.n_channels = n;
  cfg.device = -1;
  iqd_t *e = nullptr;
  int rc = iqd_create(&cfg, &e);
  if (rc != IQD_OK) {
    fprintf(stderr, "iqdemod_wide: iqd_create: %s\n", iqd_strerror(rc));
    return 1;
  }
  iqd_channelizer_config zc{};
  zc.n_sources = 1;
  zc.n_channels = n;
  zc.decimation = m;
  zc.decimation_den = den;
  iqd_channelizer_t *z = nullptr;
  rc = iqd_channelizer_create(e, &zc, &z);
  if (rc == IQD_OK) rc = iqd_channelizer_set_channels(z, 0, n, source.data(), inc.data(), shift.data());
  for (uint32_t c = 0; c < n && rc == IQD_OK; c++) rc = iqd_set_mode(e, c, 1, (int)modes[c % modes.size()]);
  if (rc == IQD_OK) rc = iqd_set_rotation(e, 0, n, rotation);
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
  const size_t block = 32768 / den * (size_t)m, call = blocks * block, unit = 64 * (size_t)m;
  std::vector<uint8_t> wide(call);
  std::vector<int16_t> pcm((size_t)n * call / m * den / 64);
  std::vector<uint32_t> count(n);
  std::vector<uint8_t> open((size_t)n * blocks);
  uint64_t block_no = 0;
  int status = 0;
  // one accept of `bytes` (whole engine blocks, or ONE short block: include/iqdemod.h), its PCM and its log lines out
  auto feed = [&](const uint8_t *p, size_t bytes) {
    const size_t nblk = bytes % block == 0 ? bytes / block : 1;
    int r = iqd_accept_wideband(e, z, 0, p, bytes, pcm.data(), count.data(), nullptr, flog ? open.data() : nullptr);
    if (r == IQD_OK && flog) {
      trace.resize((size_t)n * nblk);
      r = iqd_get_frequency_trace(e, 0, n, trace.data(), nblk);
    }
    if (r != IQD_OK) {
      fprintf(stderr, "iqdemod_wide: accept: %s (%s)\n", iqd_strerror(r), iqd_last_error(e));
      status = 3;
      return false;
    }
    const size_t row = bytes / m * den / 64;
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
  for (FILE *s : sinks) fclose(s);
  iqd_channelizer_destroy(z);
  iqd_destroy(e);
  return status;
}
