// PCM packet decoder of libiqdemod.so (include/iqdemod_fsk.h: iqd_fsk_*), on the engine's stream.  Kernels: iqd_fsk.hip.
// Here: the config's ranges, the correlators' coefficients, the call's sizes and arrays and the two launches, the host-only
// helpers; the skeleton around them is iqd_obj_host.h and its PCM part.
#include "iqd_obj_host.h"
#include "iqd_chan.h"
#include "iqd_fsk.h"
#include "iqdemod_fsk.h"

static_assert(sizeof(iqd_fsk_frame) == iqd::FSK_RECORD_BYTES && sizeof(iqd_fsk_state) == iqd::FSK_STATE_BYTES &&
              sizeof(iqd::FskState) == iqd::FSK_STATE_BYTES && sizeof(iqd_fsk_config) == 64, "the ABI's records");
static_assert(iqd::FSK_MAX_N == iqd::PCM_MAX_N, "the kernels' limit of n and row_stride");

struct iqd_fsk {
    iqd_t *e = nullptr;
    iqd::FskLaunch launch{};     // the object's half filled at create
    DevBuf state, hist, buf, dec;
    DevBuf st_pcm, st_count, st_nbits, st_bits, st_nframes, st_frames, st_bytes;
};

namespace {

struct FskSizes { size_t F, Bw, Bc; };

FskSizes fsk_sizes(const iqd_fsk *t, size_t n)
{
    const uint64_t mb = fsk_maxbits(n, t->launch.baud_inc, t->launch.loop_shift);
    if (n == 0) return {0, 0, 0};
    return {(size_t)(mb / (8 * t->launch.min_len + 8) + 1), (size_t)((mb + 31) / 32), (size_t)((t->launch.max_len + mb / 8 + 15) / 16 * 16)};
}

}  // namespace

extern "C" {

int iqd_fsk_create(iqd_t *e, const iqd_fsk_config *cfg, iqd_fsk_t **out)
{
    int rc = pcm_create_check(e, cfg, out, IQD_FSK_ABI_VERSION, __func__);
    if (rc != IQD_OK) return rc;
    const uint32_t W = cfg->corr_len;
    if (W < FSK_MIN_W || W > FSK_MAX_W) return e->fail(IQD_EINVAL, "iqd_fsk_create: corr_len (%u) must be 2 .. 64", W);
    if (cfg->baud_inc < (1u << 20) || cfg->baud_inc >= (1u << 31))
        return e->fail(IQD_EINVAL, "iqd_fsk_create: baud_inc (%u) must be 2^20 .. 2^31 - 1", cfg->baud_inc);
    if (cfg->loop_shift < 1 || cfg->loop_shift > 8) return e->fail(IQD_EINVAL, "iqd_fsk_create: loop_shift (%u) must be 1 .. 8", cfg->loop_shift);
    if (cfg->flags & ~IQD_FSK_NRZI) return e->fail(IQD_EINVAL, "iqd_fsk_create: flags (0x%x) has bits other than IQD_FSK_NRZI", cfg->flags);
    for (uint32_t k = 0; cfg->window && k < W; k++)
        if (cfg->window[k] > (int)FSK_MAX_WINDOW || cfg->window[k] < -(int)FSK_MAX_WINDOW)
            return e->fail(IQD_EINVAL, "iqd_fsk_create: window[%u] is %d: |w| must be 32512 at most", k, cfg->window[k]);
    if (cfg->min_len < 3 || cfg->min_len > cfg->max_len)
        return e->fail(IQD_EINVAL, "iqd_fsk_create: min_len (%u) must be 3 .. max_len (%u)", cfg->min_len, cfg->max_len);
    if (cfg->max_len > FSK_MAX_LEN) return e->fail(IQD_EINVAL, "iqd_fsk_create: max_len (%u) must be 1024 at most", cfg->max_len);
    if ((rc = obj_reserved_check(e, cfg->reserved, __func__)) != IQD_OK) return rc;

    iqd_fsk *t = new (std::nothrow) iqd_fsk;
    if (!t) return IQD_ENOMEM;
    t->e = e;
    FskLaunch &a = t->launch;
    std::vector<int16_t> phasor(8192);
    chz_phasor_table(phasor.data());
    for (uint32_t h = 0; h < 4; h++) {
        const uint32_t inc = h < 2 ? cfg->mark_inc : cfg->space_inc;
        for (uint32_t k = 0; k < W; k++) {
            const int32_t w = cfg->window ? cfg->window[k] : (int32_t)FSK_MAX_WINDOW;
            a.coef[h][k] = (int8_t)((w * (int32_t)phasor[2 * ((uint32_t)(k * inc) >> 20) + (h & 1)] + (1 << 22)) >> 23);
        }
    }
    a.n_channels = cfg->n_channels; a.W = W; a.baud_inc = cfg->baud_inc; a.loop_shift = cfg->loop_shift;
    a.nrzi = cfg->flags & IQD_FSK_NRZI; a.min_len = cfg->min_len; a.max_len = cfg->max_len;
    (void)hipSetDevice(e->device);
    const size_t C = a.n_channels;
    if (t->state.ensure(C * sizeof(FskState)) != hipSuccess || t->hist.ensure(C * FSK_HIST * sizeof(int16_t)) != hipSuccess ||
        t->buf.ensure(C * FSK_BUF_BYTES) != hipSuccess)
        rc = e->fail(IQD_ENOMEM, "iqd_fsk_create: no device memory for the state of %u channels", a.n_channels);
    if (rc == IQD_OK) {
        a.state = t->state.as<FskState>(); a.hist = t->hist.as<int16_t>(); a.buf = t->buf.as<uint32_t>();
        rc = iqd_fsk_reset(t);
    }
    if (rc != IQD_OK) {
        (void)hipStreamSynchronize(e->stream);
        delete t;
        return rc;
    }
    *out = t;
    return IQD_OK;
}

void iqd_fsk_destroy(iqd_fsk_t *t) { obj_destroy(t); }

// the cleared state is all zeros: the clock, NRZI, the deframer, the counters and the carried samples (x[j] = 0 for j < 0);
// the bit buffer needs no clearing: nbits = 0
int iqd_fsk_reset(iqd_fsk_t *t)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    (void)hipSetDevice(e->device);
    HIP_COPY(e, hipMemsetAsync(t->state.p, 0, (size_t)t->launch.n_channels * sizeof(FskState), e->stream));
    HIP_COPY(e, hipMemsetAsync(t->hist.p, 0, (size_t)t->launch.n_channels * FSK_HIST * sizeof(int16_t), e->stream));
    return IQD_OK;
}

size_t iqd_fsk_max_frames(const iqd_fsk_t *t, size_t n) { return t && n <= PCM_MAX_N ? fsk_sizes(t, n).F : 0; }
size_t iqd_fsk_max_bit_words(const iqd_fsk_t *t, size_t n) { return t && n <= PCM_MAX_N ? fsk_sizes(t, n).Bw : 0; }
size_t iqd_fsk_max_bytes(const iqd_fsk_t *t, size_t n) { return t && n <= PCM_MAX_N ? fsk_sizes(t, n).Bc : 0; }

int iqd_fsk_get_state(iqd_fsk_t *t, uint32_t channel, iqd_fsk_state *state)
{
    return t ? pcm_get_state(t->e, t->state.as<FskState>(), t->launch.n_channels, channel, state, __func__) : IQD_EINVAL;
}

// the call's arrays, as run stages them and run_device wants them aligned; count and bits may be left out
static ObjArgs<7> fsk_args(iqd_fsk_t *t, const void *pcm, size_t row_stride, const void *count, size_t n, void *n_bits, void *bits,
                           void *n_frames, void *frames, void *bytes)
{
    const size_t C = t->launch.n_channels;
    const FskSizes z = n <= PCM_MAX_N ? fsk_sizes(t, n) : FskSizes{0, 0, 0};
    return {{{"pcm", pcm, C * row_stride * sizeof(int16_t), &t->st_pcm, ARG_IN, 2},
             {"count", count, C * sizeof(uint32_t), &t->st_count, ARG_IN, 4, ARG_OPTIONAL},
             {"n_bits", n_bits, C * sizeof(uint32_t), &t->st_nbits, ARG_OUT, 4},
             {"bits", bits, C * z.Bw * sizeof(uint32_t), &t->st_bits, ARG_OUT, 4, ARG_OPTIONAL},
             {"n_frames", n_frames, C * sizeof(uint32_t), &t->st_nframes, ARG_OUT, 4},
             {"frames", frames, C * z.F * sizeof(iqd_fsk_frame), &t->st_frames, ARG_OUT, 8},
             {"bytes", bytes, C * z.Bc, &t->st_bytes, ARG_OUT}}};
}

int iqd_fsk_run_device(iqd_t *e, iqd_fsk_t *t, const int16_t *pcm_dev, size_t row_stride, const uint32_t *count_dev, size_t n,
                       uint32_t *n_bits_dev, uint32_t *bits_dev, uint32_t *n_frames_dev, iqd_fsk_frame *frames_dev, uint8_t *bytes_dev)
{
    if (!t) return IQD_EINVAL;
    const ObjArgs<7> args = fsk_args(t, pcm_dev, row_stride, count_dev, n, n_bits_dev, bits_dev, n_frames_dev, frames_dev, bytes_dev);
    int rc = pcm_run_check(e, t->e, args, row_stride, n, __func__);
    if (rc == IQD_OK) rc = obj_align_check(e, args, __func__);
    if (rc != IQD_OK) return rc;
    (void)hipSetDevice(e->device);
    const FskSizes z = fsk_sizes(t, n);
    FskLaunch a = t->launch;
    a.n = (uint32_t)n; a.Dw = (uint32_t)((n + 31) / 32);
    // the decision words: scratch of the object, grown to the largest call so far (no allocation per call once it is there)
    if (n && t->dec.ensure((size_t)a.n_channels * a.Dw * sizeof(uint32_t)) != hipSuccess)
        return e->fail(IQD_ENOMEM, "iqd_fsk_run_device: no device memory for the decisions of %zu samples", n);
    a.dec = t->dec.as<uint32_t>();
    a.pcm = pcm_dev; a.count = count_dev; a.row_stride = row_stride;
    a.F = (uint32_t)z.F; a.Bw = (uint32_t)z.Bw; a.Bc = (uint32_t)z.Bc;
    a.n_bits = n_bits_dev; a.bits = bits_dev; a.n_frames = n_frames_dev; a.frames = (uint32_t *)frames_dev; a.bytes = bytes_dev;
    if (n) HIP_LAUNCH(e, launch_fsk_decide(a, e->stream));
    HIP_LAUNCH(e, launch_fsk_walk(a, e->stream));
    return IQD_OK;
}

int iqd_fsk_run(iqd_t *e, iqd_fsk_t *t, const int16_t *pcm, size_t row_stride, const uint32_t *count, size_t n, uint32_t *n_bits,
                uint32_t *bits, uint32_t *n_frames, iqd_fsk_frame *frames, uint8_t *bytes)
{
    if (!t) return IQD_EINVAL;
    const ObjArgs<7> args = fsk_args(t, pcm, row_stride, count, n, n_bits, bits, n_frames, frames, bytes);
    int rc = pcm_run_check(e, t->e, args, row_stride, n, __func__);
    if (rc != IQD_OK) return rc;
    return obj_staged_run(e, args, [&] {
        return iqd_fsk_run_device(e, t, t->st_pcm.as<const int16_t>(), row_stride, count ? t->st_count.as<const uint32_t>() : nullptr, n,
                                  t->st_nbits.as<uint32_t>(), bits ? t->st_bits.as<uint32_t>() : nullptr, t->st_nframes.as<uint32_t>(),
                                  t->st_frames.as<iqd_fsk_frame>(), t->st_bytes.as<uint8_t>());
    });
}

int iqd_fsk_phase_inc(uint64_t freq_mhz, uint32_t rate_hz, uint32_t *d) { return pcm_phase_inc(freq_mhz, rate_hz, d); }

int iqd_fsk_afsk1200(uint32_t rate_hz, iqd_fsk_config *cfg)
{
    if (!cfg) return IQD_EINVAL;
    iqd_fsk_config c{};
    if (iqd_fsk_phase_inc(1200000, rate_hz, &c.mark_inc) != IQD_OK || iqd_fsk_phase_inc(2200000, rate_hz, &c.space_inc) != IQD_OK ||
        iqd_fsk_phase_inc(1200000, rate_hz, &c.baud_inc) != IQD_OK || c.baud_inc < (1u << 20) || c.baud_inc >= (1u << 31))
        return IQD_EINVAL;
    c.abi_version = IQD_FSK_ABI_VERSION;
    c.corr_len = 8; c.loop_shift = 3; c.flags = IQD_FSK_NRZI; c.min_len = 17; c.max_len = 512;
    *cfg = c;
    return IQD_OK;
}

}  // extern "C"
