// The band spectrum of libiqdemod.so (include/iqdemod.h: iqd_spectrum_*), on the engine's stream.  Kernel: iqd_spectrum.hip.
// Here: the window and the matrix packing, the config's and the lengths' refusals, the call's arrays and the launch; the skeleton
// around them is iqd_band_host.h.
#include "iqd_band_host.h"
#include "iqd_chan.h"
#include "iqd_spectrum.h"

struct iqd_spectrum {
    iqd_t *e = nullptr;
    uint32_t n_src = 0, n = 0, fmt = 0;
    DevBufExact amat;
    DevBuf st_in, st_out;
};

static_assert(SPC_MIN_BINS == BAND_MIN_BINS && SPC_MAX_BINS == BAND_MAX_BINS, "the shared refusals' bounds");

// the window's bounds (include/iqdemod.h): the first entry out of range, n if the sum is, -1 if all hold
static int64_t spectrum_window_bad(const int16_t *w, uint32_t n)
{
    int64_t sum = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (w[i] > 32639 || w[i] < -32639) return i;
        sum += abs((int)w[i]);
    }
    return 256 * sum <= 2147483647ll - 255 ? -1 : (int64_t)n;
}

static void spectrum_default_window(const int16_t *phasor, uint32_t n, int16_t *out)
{
    for (uint32_t sh = 2;; sh++) {
        int64_t sum = 0;
        for (uint32_t i = 0; i < n; i++) {
            out[i] = (int16_t)((32767 - (int32_t)phasor[2 * ((2 * i + 1) * (2048 / n))]) >> sh);
            sum += out[i];
        }
        if (256 * sum <= 2147483647ll - 255) return;
    }
}

namespace iqd {

void spc_pack(const int16_t *w, const int16_t *phasor, uint32_t n, uint8_t *amat)
{
    const uint32_t steps = n / 32;
    for (uint32_t k = 0; k < n; k++) {                       // bin k', q = k' - n / 2 (mod n)
        const uint32_t tile = k / SPC_TILE_BINS, rho = k % SPC_TILE_BINS, qn = (k + n / 2) % n;
        for (uint32_t kappa = 0; kappa < 2 * n; kappa++) {
            const uint32_t s = kappa / 2, i = (uint32_t)(((uint64_t)qn * s) % n) * (CHZ_PHASOR / n);
            const int32_t c = ((int32_t)w[s] * phasor[2 * i] + (1 << 14)) >> 15;
            const int32_t sn = ((int32_t)w[s] * phasor[2 * i + 1] + (1 << 14)) >> 15;
            const int32_t v[2] = {kappa & 1 ? sn : c, kappa & 1 ? c : -sn};   // rail r: (c, s, ...), rail i: (-s, c, ...)
            const uint32_t step = kappa / 64, g = (kappa % 64) / 16, j = kappa % 16;
            for (uint32_t rail = 0; rail < 2; rail++) {
                const int32_t hi = (v[rail] + 128) >> 8, lo = v[rail] - 256 * hi;   // |v| <= 32639: hi in [-127, 127]
                const size_t at = ((((size_t)tile * steps + step) * SPC_PLANES + 2 * rail) * 64 + rho + 16 * g) * 16 + j;
                amat[at] = (uint8_t)(int8_t)lo;
                amat[at + 64 * 16] = (uint8_t)(int8_t)hi;
            }
        }
    }
}

}  // namespace iqd

extern "C" {

int iqd_spectrum_default_window(uint32_t n_bins, int16_t *out)
{
    if (!out || !band_bins_ok(n_bins)) return IQD_EINVAL;
    std::vector<int16_t> phasor(2 * CHZ_PHASOR);
    chz_phasor_table(phasor.data());
    spectrum_default_window(phasor.data(), n_bins, out);
    return IQD_OK;
}

int iqd_spectrum_full_scale(const int16_t *window, uint32_t n_bins, uint32_t *p_fs)
{
    if (!p_fs || !band_bins_ok(n_bins)) return IQD_EINVAL;
    std::vector<int16_t> w(n_bins);
    if (window) {
        if (spectrum_window_bad(window, n_bins) >= 0) return IQD_EINVAL;
        memcpy(w.data(), window, n_bins * sizeof(int16_t));
    } else {
        iqd_spectrum_default_window(n_bins, w.data());
    }
    int64_t sum = 0;
    for (uint32_t i = 0; i < n_bins; i++) sum += (32767 * (int32_t)w[i] + (1 << 14)) >> 15;
    const int64_t a = (127 * sum + (1 << 15)) >> 16;      // |a| < 2^16
    *p_fs = (uint32_t)(a * a);
    return IQD_OK;
}

int iqd_spectrum_create(iqd_t *e, const iqd_spectrum_config *cfg, iqd_spectrum_t **out)
{
    int rc = obj_create_check(e, cfg, out, __func__);
    if (rc != IQD_OK) return rc;
    if (cfg->n_sources == 0) return e->fail(IQD_EINVAL, "iqd_spectrum_create: n_sources is 0");
    if ((rc = band_bins_check(e, cfg->n_bins, __func__)) != IQD_OK) return rc;
    if (cfg->sample_format == IQD_WIDE_S16)
        return e->fail(IQD_EINVAL, "iqd_spectrum_create: sample_format IQD_WIDE_S16 is not supported (IQD_WIDE_U8 or IQD_WIDE_S8)");
    if (cfg->sample_format > IQD_WIDE_S16)
        return e->fail(IQD_EINVAL, "iqd_spectrum_create: sample_format (%u) is none of IQD_WIDE_U8, IQD_WIDE_S8", cfg->sample_format);
    if ((rc = obj_reserved_check(e, cfg->reserved, __func__)) != IQD_OK) return rc;
    const uint32_t n = cfg->n_bins;
    if (cfg->window) {
        const int64_t bad = spectrum_window_bad(cfg->window, n);
        if (bad == (int64_t)n) return e->fail(IQD_EINVAL, "iqd_spectrum_create: window: 256 sum |w| is above 2^31 - 256");
        if (bad >= 0) return e->fail(IQD_EINVAL, "iqd_spectrum_create: window[%lld] = %d is outside [-32639, 32639]", (long long)bad, (int)cfg->window[bad]);
    }
    (void)hipSetDevice(e->device);
    iqd_spectrum *s = new (std::nothrow) iqd_spectrum;
    if (!s) return IQD_ENOMEM;
    s->e = e; s->n_src = cfg->n_sources; s->n = n; s->fmt = cfg->sample_format;
    std::vector<int16_t> phasor(2 * CHZ_PHASOR), w(n);
    chz_phasor_table(phasor.data());
    if (cfg->window) memcpy(w.data(), cfg->window, n * sizeof(int16_t));
    else spectrum_default_window(phasor.data(), n, w.data());
    std::vector<uint8_t> amat(spc_amat_bytes(n));
    spc_pack(w.data(), phasor.data(), n, amat.data());
    bool ok = s->amat.ensure(amat.size()) == hipSuccess;
    ok = ok && hipMemcpy(s->amat.p, amat.data(), amat.size(), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) { iqd_spectrum_destroy(s); return e->fail(IQD_ENOMEM, "spectrum allocation failed"); }
    *out = s;
    return IQD_OK;
}

void iqd_spectrum_destroy(iqd_spectrum_t *s) { obj_destroy(s); }

// the call's arrays, as run stages them: [n_sources] captures in, [n_sources][n_blocks][n_bins] powers out
static ObjArgs<2> spectrum_args(iqd_spectrum_t *s, const void *wide, size_t bytes_per_source, uint32_t frames, void *power)
{
    const size_t n_blocks = frames ? bytes_per_source / ((size_t)2 * s->n * frames) : 0;
    return {{{"wide", wide, (size_t)s->n_src * bytes_per_source, &s->st_in, ARG_IN},
             {"power", power, (size_t)s->n_src * n_blocks * s->n * sizeof(uint32_t), &s->st_out, ARG_OUT}}};
}

// a call is whole blocks of frames_per_block frames: the lengths' refusals are the spectrum's own
static int spectrum_run_check(iqd_spectrum_t *s, const ObjArgs<2> &args, size_t bytes_per_source, uint32_t frames, const char *who)
{
    iqd_t *e = s->e;
    int rc = obj_null_check(e, args, who);
    if (rc != IQD_OK) return rc;
    if (frames == 0 || frames > SPC_MAX_FRAMES) return e->fail(IQD_EINVAL, "%s: frames_per_block (%u) must be 1 .. 2^24", who, frames);
    const size_t blk = (size_t)2 * s->n * frames;
    if (bytes_per_source == 0 || bytes_per_source % blk != 0)
        return e->fail(IQD_EINVAL, "%s: bytes_per_source (%zu) must be a positive multiple of 2 x n_bins x frames_per_block (%zu)", who,
                       bytes_per_source, blk);
    const uint64_t n_wgs = (uint64_t)(bytes_per_source / blk) * s->n_src * (s->n / SPC_WG_BINS);
    if (bytes_per_source / blk > 0xffffffffull || n_wgs > 0x7fffffffull)
        return e->fail(IQD_EINVAL, "%s: bytes_per_source (%zu): n_sources x n_blocks x n_bins / 64 is more than one launch covers", who,
                       bytes_per_source);
    return IQD_OK;
}

int iqd_spectrum_run_device(iqd_spectrum_t *s, const void *wide_dev, size_t bytes_per_source, uint32_t frames_per_block,
                            uint32_t *power_dev)
{
    if (!s) return IQD_EINVAL;
    iqd_t *e = s->e;
    const ObjArgs<2> args = spectrum_args(s, wide_dev, bytes_per_source, frames_per_block, power_dev);
    int rc = spectrum_run_check(s, args, bytes_per_source, frames_per_block, __func__);
    if (rc == IQD_OK) rc = obj_align_check(e, args, __func__);
    if (rc != IQD_OK) return rc;
    (void)hipSetDevice(e->device);
    SpcLaunch a{};
    a.wide = (const uint8_t *)wide_dev; a.power = power_dev; a.amat = s->amat.as<const uint4>();
    a.bytes_per_source = bytes_per_source; a.n = s->n; a.n_sources = s->n_src;
    a.n_blocks = (uint32_t)(bytes_per_source / ((size_t)2 * s->n * frames_per_block)); a.frames = frames_per_block;
    a.flip = s->fmt == IQD_WIDE_U8 ? 1u : 0u;
    HIP_LAUNCH(e, launch_spectrum(a, e->stream));
    return IQD_OK;
}

int iqd_spectrum_run(iqd_spectrum_t *s, const void *wide, size_t bytes_per_source, uint32_t frames_per_block, uint32_t *power)
{
    if (!s) return IQD_EINVAL;
    const ObjArgs<2> args = spectrum_args(s, wide, bytes_per_source, frames_per_block, power);
    int rc = spectrum_run_check(s, args, bytes_per_source, frames_per_block, __func__);
    if (rc != IQD_OK) return rc;
    return obj_staged_run(s->e, args, [&] {
        return iqd_spectrum_run_device(s, s->st_in.p, bytes_per_source, frames_per_block, s->st_out.as<uint32_t>());
    });
}

}  // extern "C"
