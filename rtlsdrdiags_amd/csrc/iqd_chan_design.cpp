// Wideband channelizer, host only (include/iqdemod.h): the phasor table, the default prototype and the rule for the
// decimation ratio, a channel's tuning, the window sizes.  No HIP call.
#include <math.h>

#include <algorithm>
#include <vector>

#include "iqd_chan_layout.h"

namespace iqd {

void chz_phasor_table(int16_t *out)
{
    for (int i = 0; i < (int)CHZ_PHASOR; i++) {
        const double ph = 2.0 * M_PI * i / CHZ_PHASOR;
        out[2 * i] = (int16_t)lrint(32767.0 * cos(ph));
        out[2 * i + 1] = (int16_t)lrint(32767.0 * sin(ph));
    }
}

bool chz_ratio_ok(uint32_t p, uint32_t q)
{
    if (q != 1 && q != 2 && q != 4 && q != 8) return false;
    if (q > 1 && p % 2 == 0) return false;
    return p >= 2 * q && p <= 64 * q;
}

static double bessel_i0(double x)
{
    double sum = 1, term = 1;
    for (int k = 1; k < 200; k++) {
        const double f = x / (2.0 * k);
        term *= f * f;
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

}  // namespace iqd

using namespace iqd;

extern "C" {

int iqd_channelizer_phasor_table(int16_t out[8192])
{
    if (!out) return IQD_EINVAL;
    chz_phasor_table(out);
    return IQD_OK;
}

// Kaiser-windowed sinc (beta 5, cut-off 124 kHz at the wide rate, 13 M + 1 taps), quantised to Q15; the centre tap takes
// up the rounding so that the DC gain is exactly 32768.  Stopband from 156 kHz >= 53 dB, passband +-100 kHz ripple
// 0.32 dB (tests/test_chan_host.py checks the quantised taps for M in 2..64).
int iqd_channelizer_default_taps(uint32_t decimation, int16_t *out, uint32_t capacity)
{
    return iqd_channelizer_default_taps_q(decimation, 1, out, capacity);
}

// The same design at the rate 256000 P, quantised per branch r (taps r, r + Q, ...): each branch is normalised to DC gain
// 32768 on its own and its first largest tap takes up the rounding, so the gain does not ripple at the output rate.
int iqd_channelizer_default_taps_q(uint32_t decimation, uint32_t den, int16_t *out, uint32_t capacity)
{
    if (den == 0) den = 1;
    if (!chz_ratio_ok(decimation, den) || (!out && capacity)) return IQD_EINVAL;
    const uint32_t n = 13 * decimation + 1;
    const double fc = 124.0 / (256.0 * decimation), beta = 5.0, i0b = bessel_i0(beta);
    std::vector<double> w(n);
    for (uint32_t i = 0; i < n; i++) {
        const double x = (double)i - (n - 1) / 2.0, r = 2.0 * i / (n - 1) - 1.0;
        const double sinc = x == 0 ? 1.0 : sin(2 * M_PI * fc * x) / (2 * M_PI * fc * x);
        w[i] = 2 * fc * sinc * bessel_i0(beta * sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    }
    std::vector<int32_t> q(n);
    for (uint32_t br = 0; br < den; br++) {
        double sum = 0, peak = 0;
        for (uint32_t i = br; i < n; i += den) {
            sum += w[i];
            peak = std::max(peak, fabs(w[i]));
        }
        int32_t qs = 0;
        uint32_t at = br;                          // the first largest tap (two equal ones: a rounding apart at most)
        bool found = false;
        for (uint32_t i = br; i < n; i += den) {
            qs += q[i] = (int32_t)lrint(w[i] / sum * 32768.0);
            if (!found && fabs(w[i]) >= peak * (1 - 1e-12)) {
                at = i;
                found = true;
            }
        }
        q[at] += 32768 - qs;
    }
    for (uint32_t i = 0; i < n && i < capacity; i++) out[i] = (int16_t)q[i];
    return (int)n;
}

// chz_track_window_outputs as a host-only function
uint32_t iqd_channelizer_track_window_outputs(uint32_t decimation, uint32_t n_taps)
{
    if (decimation < 2 || decimation > 64 || n_taps < 1 || n_taps > 1024) return 0;
    return chz_track_window_outputs(decimation, (n_taps + 31) / 32 * 32);
}

// chz_window_outputs as a host-only function (the window's fit in LDS is checked on it for every M)
uint32_t iqd_channelizer_window_outputs(uint32_t decimation, uint32_t n_taps, uint32_t sample_format)
{
    if (decimation < 2 || decimation > 64 || n_taps < 1 || n_taps > 1024 || sample_format > IQD_WIDE_S16) return 0;
    return chz_window_outputs(decimation, (n_taps + 31) / 32 * 32, 1, sample_format == IQD_WIDE_S16 ? 2 : 1);
}

int iqd_channelizer_tuning(uint32_t decimation, uint64_t source_centre_hz, uint64_t station_hz, int rotation, uint32_t *inc)
{
    if (decimation < 2 || decimation > 64 || rotation < -1 || rotation > 1 || !inc) return IQD_EINVAL;
    return chz_tuning(decimation, source_centre_hz, station_hz, rotation, inc) ? IQD_OK : IQD_EINVAL;
}

}  // extern "C"
