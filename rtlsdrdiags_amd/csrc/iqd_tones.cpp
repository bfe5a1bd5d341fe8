// PCM tone bank of libiqdemod.so (include/iqdemod_tones.h: iqd_tones_*), on the engine's stream.  Kernels: iqd_tones.hip.
// Here: the config's ranges, the coefficient tables as MFMA operands, the call's arrays and the two launches, the host-only
// helpers; the skeleton around them is iqd_obj_host.h and its PCM part.
#include "iqd_obj_host.h"
#include "iqd_chan.h"
#include "iqd_tones.h"
#include "iqdemod_tones.h"

static_assert(sizeof(iqd_tones_frame) == iqd::TON_RECORD_BYTES && sizeof(iqd_tones_state) == iqd::TON_STATE_BYTES &&
              sizeof(iqd::TonState) == iqd::TON_STATE_BYTES && sizeof(iqd_tones_config) == 72, "the ABI's records");
static_assert(iqd::TON_MAX_N == iqd::PCM_MAX_N, "the kernels' limit of n and row_stride");

struct iqd_tones {
    iqd_t *e = nullptr;
    uint32_t n_channels = 0, L = 0, T = 0;
    uint64_t min_power = 0;
    uint32_t ratio_q8 = 0, energy_q8 = 0, open = 0, hold = 0;
    DevBuf amat, gsum, state, frame;
    DevBuf st_pcm, st_count, st_nframes, st_frames, st_power;
};

namespace {

void ton_default_window(uint32_t L, const int16_t *phasor, int16_t *w)
{
    for (uint32_t n = 0; n < L; n++) w[n] = (int16_t)((32767 - phasor[2 * (((2 * n + 1) * 2048u) / L)]) >> 2);
}

// The coefficients c_t[n], s_t[n] as the A operands of ton_frames_kernel (iqd_tones.h: TonLaunch::amat) and the rows' sums:
// row 2 t = c_t, 2 t + 1 = s_t; each value v = 256 hi + lo' + 128, hi = v >> 8, lo' = (v & 255) - 128; zeros in the padding.
void ton_pack(uint32_t L, uint32_t T, const uint32_t *inc, const int16_t *w, const int16_t *phasor, std::vector<uint8_t> &amat,
              std::vector<int32_t> &gsum)
{
    const uint32_t NQ = ton_padded(L) / 64, NT = ton_row_tiles(T);
    amat.assign((size_t)NT * NQ * 2 * 64 * 16, 0);
    gsum.assign((size_t)NT * TON_TILE_ROWS, 0);
    for (uint32_t t = 0; t < T; t++)
        for (uint32_t n = 0; n < L; n++) {
            const uint32_t i = (uint32_t)(n * inc[t]) >> 20;
            for (uint32_t h = 0; h < 2; h++) {
                const int32_t v = (w[n] * (int32_t)phasor[2 * i + h] + 16384) >> 15;
                const uint32_t r = 2 * t + h, rt = r / TON_TILE_ROWS, q = n / 64, lane = r % TON_TILE_ROWS + 16 * (n % 64 / 16), j = n % 16;
                const size_t at = (((size_t)rt * NQ + q) * 2 * 64 + lane) * 16 + j;
                amat[at] = (uint8_t)(v >> 8);
                amat[at + 64 * 16] = (uint8_t)((v & 255) ^ 128);
                gsum[r] += v;
            }
        }
}

int ton_upload(iqd_t *e, DevBuf &b, const void *src, size_t bytes, const char *who)
{
    if (b.ensure(bytes) != hipSuccess) return e->fail(IQD_ENOMEM, "%s: no device memory for %zu bytes", who, bytes);
    HIP_COPY(e, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, e->stream));
    return IQD_OK;
}

size_t ton_frames(const iqd_tones *t, size_t n) { return (n + t->L - 1) / t->L; }

}  // namespace

extern "C" {

int iqd_tones_create(iqd_t *e, const iqd_tones_config *cfg, iqd_tones_t **out)
{
    int rc = pcm_create_check(e, cfg, out, IQD_TONES_ABI_VERSION, __func__);
    if (rc != IQD_OK) return rc;
    const uint32_t L = cfg->frame_len, T = cfg->n_tones;
    if (L < TON_MIN_L || L > TON_MAX_L || L % 32) return e->fail(IQD_EINVAL, "iqd_tones_create: frame_len (%u) must be a multiple of 32, 32 .. 8192", L);
    if (T == 0 || T > TON_MAX_T) return e->fail(IQD_EINVAL, "iqd_tones_create: n_tones (%u) must be 1 .. 64", T);
    if (!cfg->phase_inc) return e->fail(IQD_EINVAL, "iqd_tones_create: phase_inc is NULL");
    for (uint32_t n = 0; cfg->window && n < L; n++)
        if (cfg->window[n] == -32768) return e->fail(IQD_EINVAL, "iqd_tones_create: window[%u] is -32768: |w| must be 32767 at most", n);
    if (cfg->ratio_q8 < 256 || cfg->ratio_q8 > 65535) return e->fail(IQD_EINVAL, "iqd_tones_create: ratio_q8 (%u) must be 256 .. 65535", cfg->ratio_q8);
    if (cfg->energy_q8 > (1u << 20)) return e->fail(IQD_EINVAL, "iqd_tones_create: energy_q8 (%u) must be 0 .. 2^20", cfg->energy_q8);
    if (cfg->open < 1 || cfg->open > 255) return e->fail(IQD_EINVAL, "iqd_tones_create: open (%u) must be 1 .. 255", cfg->open);
    if (cfg->hold > 255) return e->fail(IQD_EINVAL, "iqd_tones_create: hold (%u) must be 0 .. 255", cfg->hold);
    if ((rc = obj_reserved_check(e, cfg->reserved, __func__)) != IQD_OK) return rc;

    std::vector<int16_t> phasor(8192), w(L);
    chz_phasor_table(phasor.data());
    if (cfg->window) std::copy(cfg->window, cfg->window + L, w.begin());
    else ton_default_window(L, phasor.data(), w.data());
    std::vector<uint8_t> amat;
    std::vector<int32_t> gsum;
    ton_pack(L, T, cfg->phase_inc, w.data(), phasor.data(), amat, gsum);

    iqd_tones *t = new (std::nothrow) iqd_tones;
    if (!t) return IQD_ENOMEM;
    t->e = e; t->n_channels = cfg->n_channels; t->L = L; t->T = T;
    t->min_power = cfg->min_power; t->ratio_q8 = cfg->ratio_q8; t->energy_q8 = cfg->energy_q8; t->open = cfg->open; t->hold = cfg->hold;
    (void)hipSetDevice(e->device);
    rc = ton_upload(e, t->amat, amat.data(), amat.size(), __func__);
    if (rc == IQD_OK) rc = ton_upload(e, t->gsum, gsum.data(), gsum.size() * sizeof(int32_t), __func__);
    if (rc == IQD_OK && (t->state.ensure((size_t)t->n_channels * sizeof(TonState)) != hipSuccess ||
                         t->frame.ensure((size_t)t->n_channels * L * sizeof(int16_t)) != hipSuccess))
        rc = e->fail(IQD_ENOMEM, "iqd_tones_create: no device memory for the state of %u channels", t->n_channels);
    if (rc == IQD_OK) rc = iqd_tones_reset(t);
    if (rc == IQD_OK && hipStreamSynchronize(e->stream) != hipSuccess)   // the uploads read this function's vectors
        rc = e->fail(IQD_EHIP, "iqd_tones_create: the upload failed");
    if (rc != IQD_OK) {
        (void)hipStreamSynchronize(e->stream);
        delete t;
        return rc;
    }
    *out = t;
    return IQD_OK;
}

void iqd_tones_destroy(iqd_tones_t *t) { obj_destroy(t); }

// the cleared state: tone = cand = -1, the rest 0 (the open frame's samples need no clearing: fill = 0)
int iqd_tones_reset(iqd_tones_t *t)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    (void)hipSetDevice(e->device);
    HIP_LAUNCH(e, launch_tones_reset(t->state.as<TonState>(), t->n_channels, e->stream));
    return IQD_OK;
}

size_t iqd_tones_max_frames(const iqd_tones_t *t, size_t n) { return t ? ton_frames(t, n) : 0; }

int iqd_tones_get_state(iqd_tones_t *t, uint32_t channel, iqd_tones_state *state)
{
    return t ? pcm_get_state(t->e, t->state.as<TonState>(), t->n_channels, channel, state, __func__) : IQD_EINVAL;
}

// the call's arrays, as run stages them and run_device wants them aligned; count and power may be left out
static ObjArgs<5> tones_args(iqd_tones_t *t, const void *pcm, size_t row_stride, const void *count, size_t n, void *n_frames, void *frames,
                             void *power)
{
    const size_t C = t->n_channels, F = ton_frames(t, n);
    return {{{"pcm", pcm, C * row_stride * sizeof(int16_t), &t->st_pcm, ARG_IN, 2},
             {"count", count, C * sizeof(uint32_t), &t->st_count, ARG_IN, 4, ARG_OPTIONAL},
             {"n_frames", n_frames, C * sizeof(uint32_t), &t->st_nframes, ARG_OUT, 4},
             {"frames", frames, C * F * sizeof(iqd_tones_frame), &t->st_frames, ARG_OUT},
             {"power", power, C * F * t->T * sizeof(uint64_t), &t->st_power, ARG_OUT, 16, ARG_OPTIONAL}}};
}

int iqd_tones_run_device(iqd_t *e, iqd_tones_t *t, const int16_t *pcm_dev, size_t row_stride, const uint32_t *count_dev, size_t n,
                         uint32_t *n_frames_dev, iqd_tones_frame *frames_dev, uint64_t *power_dev)
{
    if (!t) return IQD_EINVAL;
    const ObjArgs<5> args = tones_args(t, pcm_dev, row_stride, count_dev, n, n_frames_dev, frames_dev, power_dev);
    int rc = pcm_run_check(e, t->e, args, row_stride, n, __func__);
    if (rc == IQD_OK) rc = obj_align_check(e, args, __func__);
    if (rc != IQD_OK) return rc;
    (void)hipSetDevice(e->device);
    TonLaunch a{};
    a.amat = t->amat.as<const uint4>(); a.gsum = t->gsum.as<const int32_t>(); a.state = t->state.as<TonState>(); a.open = t->frame.as<int16_t>();
    a.n_channels = t->n_channels; a.L = t->L; a.T = t->T;
    a.min_power = t->min_power; a.ratio_q8 = t->ratio_q8; a.energy_q8 = t->energy_q8; a.open_frames = t->open; a.hold = t->hold;
    a.pcm = pcm_dev; a.count = count_dev; a.row_stride = row_stride; a.n = (uint32_t)n; a.F = (uint32_t)ton_frames(t, n);
    a.n_frames = n_frames_dev; a.frames = (uint64_t *)frames_dev; a.power = power_dev;
    if (a.F) HIP_LAUNCH(e, launch_tones_frames(a, e->stream));
    HIP_LAUNCH(e, launch_tones_close(a, e->stream));
    return IQD_OK;
}

int iqd_tones_run(iqd_t *e, iqd_tones_t *t, const int16_t *pcm, size_t row_stride, const uint32_t *count, size_t n, uint32_t *n_frames,
                  iqd_tones_frame *frames, uint64_t *power)
{
    if (!t) return IQD_EINVAL;
    const ObjArgs<5> args = tones_args(t, pcm, row_stride, count, n, n_frames, frames, power);
    int rc = pcm_run_check(e, t->e, args, row_stride, n, __func__);
    if (rc != IQD_OK) return rc;
    return obj_staged_run(e, args, [&] {
        return iqd_tones_run_device(e, t, t->st_pcm.as<const int16_t>(), row_stride, count ? t->st_count.as<const uint32_t>() : nullptr, n,
                                    t->st_nframes.as<uint32_t>(), t->st_frames.as<iqd_tones_frame>(), power ? t->st_power.as<uint64_t>() : nullptr);
    });
}

int iqd_tones_phase_inc(uint64_t freq_mhz, uint32_t rate_hz, uint32_t *d) { return pcm_phase_inc(freq_mhz, rate_hz, d); }

int iqd_tones_default_window(uint32_t frame_len, int16_t *window)
{
    if (!window || frame_len < TON_MIN_L || frame_len > TON_MAX_L || frame_len % 32) return IQD_EINVAL;
    std::vector<int16_t> phasor(8192);
    chz_phasor_table(phasor.data());
    ton_default_window(frame_len, phasor.data(), window);
    return IQD_OK;
}

int iqd_tones_ctcss(uint32_t freq_mhz[50])
{
    static const uint16_t dhz[50] = {670,  693,  719,  744,  770,  797,  825,  854,  885,  915,  948,  974,  1000, 1035, 1072, 1109, 1148,
                                     1188, 1230, 1273, 1318, 1365, 1413, 1462, 1514, 1567, 1598, 1622, 1655, 1679, 1713, 1738, 1773, 1799,
                                     1835, 1862, 1899, 1928, 1966, 1995, 2035, 2065, 2107, 2181, 2257, 2291, 2336, 2418, 2503, 2541};
    if (!freq_mhz) return IQD_EINVAL;
    for (int i = 0; i < 50; i++) freq_mhz[i] = 100u * dhz[i];
    return IQD_OK;
}

int iqd_tones_dtmf(uint32_t freq_mhz[8])
{
    static const uint16_t hz[8] = {697, 770, 852, 941, 1209, 1336, 1477, 1633};
    if (!freq_mhz) return IQD_EINVAL;
    for (int i = 0; i < 8; i++) freq_mhz[i] = 1000u * hz[i];
    return IQD_OK;
}

}  // extern "C"
