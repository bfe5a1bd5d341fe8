// The stand-alone filter classes of libiqdemod.so (include/iqdemod.h: iqd_filter_*), on the engine's stream:
// Decimator_int16, FirFilter_int16, FirFilter and IirFilter for n_channels independent streams.  Kernels: iqd_filter.hip.
#include "iqd_engine_impl.h"
#include "iqd_filter.h"

struct iqd_filter {
    iqd_t *e = nullptr;
    int kind = 0;
    uint32_t n_ch = 0, factor = 1, n_num = 0, n_den = 0, k0 = 0, elem = 4;
    uint64_t count = 0;          // samples accepted since create / reset (the decimator's commutator phase)
    DevBuf taps, hist[2], state, st_in, st_out;
    int cur = 0;
    bool is_fir() const { return kind != IQD_FILTER_IIR_F32; }
    bool is_q15() const { return kind == IQD_FILTER_DECIMATE_I16 || kind == IQD_FILTER_FIR_I16; }
    size_t hist_bytes() const { return (size_t)n_ch * (n_num - 1) * elem; }
    size_t state_bytes() const { return (size_t)n_ch * (n_num - 1 + n_den) * sizeof(float); }
};

// the sizes a kind accepts (include/iqdemod.h); the name of the first argument out of range, or nullptr
static const char *filter_sizes_bad(int kind, uint32_t n_num, uint32_t n_den, uint32_t factor)
{
    if (kind < IQD_FILTER_DECIMATE_I16 || kind > IQD_FILTER_IIR_F32) return "kind";
    if (kind == IQD_FILTER_IIR_F32) {
        if (n_num < 1 || n_num > FLT_IIR_MAX_ORDER) return "n_num";
        if (n_den < 1 || n_den > FLT_IIR_MAX_ORDER) return "n_den";
        return factor == 1 ? nullptr : "factor";
    }
    if (n_num < 1 || n_num > FLT_MAX_TAPS) return "n_num";
    if (n_den != 0) return "n_den";
    if (kind == IQD_FILTER_DECIMATE_I16) return factor >= 1 && factor <= FLT_MAX_FACTOR ? nullptr : "factor";
    return factor == 1 ? nullptr : "factor";
}

static uint32_t clamp_free_prefix(const int16_t *hq, uint32_t n)
{
    uint32_t sum = 0, k = 0;
    for (; k < n; k++) {
        sum += (uint32_t)abs((int)hq[k]);
        if (sum > 32767) break;
    }
    return k;
}

extern "C" {

uint32_t iqd_filter_tile_samples(int kind, uint32_t n_num, uint32_t n_den, uint32_t factor)
{
    if (filter_sizes_bad(kind, n_num, n_den, factor)) return 0;
    return kind == IQD_FILTER_IIR_F32 ? FLT_IIR_TILE : FLT_WG * factor;
}

uint32_t iqd_filter_clamp_free_taps(const float *taps, uint32_t n_taps)
{
    if (!taps || n_taps == 0) return 0;
    std::vector<int16_t> hq(n_taps);
    quantize_q15(taps, (int)n_taps, hq.data());
    return clamp_free_prefix(hq.data(), n_taps);
}

int iqd_filter_create(iqd_t *e, int kind, const float *num, uint32_t n_num, const float *den, uint32_t n_den, uint32_t factor,
                      uint32_t n_channels, iqd_filter_t **out)
{
    if (!e) return IQD_EINVAL;
    if (!out) return e->fail(IQD_EINVAL, "iqd_filter_create: out is NULL");
    if (!num) return e->fail(IQD_EINVAL, "iqd_filter_create: num is NULL");
    if (const char *bad = filter_sizes_bad(kind, n_num, n_den, factor))
        return e->fail(IQD_EINVAL, "iqd_filter_create: %s out of range (kind %d, n_num %u, n_den %u, factor %u)", bad, kind, n_num,
                       n_den, factor);
    if (kind == IQD_FILTER_IIR_F32 && !den) return e->fail(IQD_EINVAL, "iqd_filter_create: den is NULL (IIR_F32 needs it)");
    if (kind != IQD_FILTER_IIR_F32 && den) return e->fail(IQD_EINVAL, "iqd_filter_create: den must be NULL for the FIR kinds");
    if (n_channels == 0) return e->fail(IQD_EINVAL, "iqd_filter_create: n_channels is 0");
    (void)hipSetDevice(e->device);
    iqd_filter *f = new (std::nothrow) iqd_filter;
    if (!f) return IQD_ENOMEM;
    f->e = e; f->kind = kind; f->n_ch = n_channels; f->factor = factor; f->n_num = n_num; f->n_den = n_den;
    f->elem = f->is_q15() ? 2 : 4;
    std::vector<uint32_t> words;
    if (f->is_q15()) {   // two taps per word (iqd_filter.h: FirLaunch::taps)
        std::vector<int16_t> hq(n_num);
        quantize_q15(num, (int)n_num, hq.data());
        f->k0 = clamp_free_prefix(hq.data(), n_num) & ~1u;
        words.assign((n_num + 1) / 2, 0u);
        for (uint32_t k = 0; k < n_num; k++) words[k / 2] |= (uint32_t)(uint16_t)hq[k] << (16 * (1 - (k & 1)));
    } else {
        words.resize(n_num + n_den);
        memcpy(words.data(), num, n_num * sizeof(float));
        if (n_den) memcpy(words.data() + n_num, den, n_den * sizeof(float));
    }
    bool ok = f->taps.ensure(words.size() * 4) == hipSuccess;
    ok = ok && hipMemcpy(f->taps.p, words.data(), words.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (f->is_fir()) {
        const size_t hb = f->hist_bytes();
        for (int b = 0; b < 2 && ok; b++) ok = f->hist[b].ensure(hb ? hb : 16) == hipSuccess;
        ok = ok && (!hb || hipMemset(f->hist[0].p, 0, hb) == hipSuccess);
    } else {
        ok = ok && f->state.ensure(f->state_bytes()) == hipSuccess;
        ok = ok && hipMemset(f->state.p, 0, f->state_bytes()) == hipSuccess;
    }
    if (!ok) { iqd_filter_destroy(f); return e->fail(IQD_ENOMEM, "filter allocation failed"); }
    *out = f;
    return IQD_OK;
}

void iqd_filter_destroy(iqd_filter_t *f)
{
    if (!f) return;
    (void)hipSetDevice(f->e->device);
    (void)hipStreamSynchronize(f->e->stream);
    delete f;
}

int iqd_filter_reset(iqd_filter_t *f)   // resetFilterState()
{
    if (!f) return IQD_EINVAL;
    (void)hipSetDevice(f->e->device);
    if (f->is_fir()) {
        if (f->hist_bytes()) HIP_TRY(f->e, hipMemsetAsync(f->hist[f->cur].p, 0, f->hist_bytes(), f->e->stream));
    } else {
        HIP_TRY(f->e, hipMemsetAsync(f->state.p, 0, f->state_bytes(), f->e->stream));
    }
    f->count = 0;
    return IQD_OK;
}

size_t iqd_filter_out_count(const iqd_filter_t *f, size_t n_in)
{
    if (!f) return 0;
    if (f->kind != IQD_FILTER_DECIMATE_I16) return n_in;
    return (size_t)((f->count % f->factor + n_in) / f->factor);
}

// the refusals of a run, before anything is queued
static int filter_run_check(iqd_filter_t *f, const void *in, size_t n_in, const void *out, const char *who)
{
    if (!f) return IQD_EINVAL;
    if (!in) return f->e->fail(IQD_EINVAL, "%s: in is NULL", who);
    if (!out) return f->e->fail(IQD_EINVAL, "%s: out is NULL", who);
    if (n_in > 0x7fffffffu) return f->e->fail(IQD_EINVAL, "%s: n_in (%zu) is above 2^31 - 1", who, n_in);
    const uint64_t n_out = iqd_filter_out_count(f, n_in);
    const uint64_t wgs = f->is_fir() ? (uint64_t)f->n_ch * ((n_out + FLT_WG - 1) / FLT_WG + 1) : 0;
    if (wgs > 0x7fffffffu) return f->e->fail(IQD_EINVAL, "%s: n_channels x n_in (%u x %zu) is more than one launch covers", who, f->n_ch, n_in);
    return IQD_OK;
}

int iqd_filter_run_device(iqd_filter_t *f, const void *in_dev, size_t n_in, void *out_dev)
{
    int rc = filter_run_check(f, in_dev, n_in, out_dev, "iqd_filter_run_device");
    if (rc != IQD_OK) return rc;
    iqd_t *e = f->e;
    if (n_in == 0) return IQD_OK;
    (void)hipSetDevice(e->device);
    if (!f->is_fir()) {
        IirLaunch a{(const float *)in_dev, (float *)out_dev, f->state.as<float>(), f->taps.as<const float>(), f->n_ch, (uint32_t)n_in,
                    f->n_num, f->n_den, ((((uintptr_t)in_dev | (uintptr_t)out_dev) % 16 == 0 && n_in % 4 == 0) ? 1u : 0u)};
        HIP_LAUNCH(e, launch_filter_iir(a, e->stream));
        f->count += n_in;
        return IQD_OK;
    }
    FirLaunch a{};
    a.in = in_dev; a.out = out_dev; a.hist = f->hist[f->cur].p; a.hist_next = f->hist[f->cur ^ 1].p;
    a.taps = f->taps.as<const uint32_t>();
    a.n_ch = f->n_ch; a.n_in = (uint32_t)n_in; a.n_out = (uint32_t)iqd_filter_out_count(f, n_in);
    a.n_taps = f->n_num; a.factor = f->factor; a.k0 = f->k0;
    a.first = f->factor - 1 - (uint32_t)(f->count % f->factor);
    a.group = a.n_out >= FLT_WG ? FLT_WG : FLT_WAVE;
    a.groups_per_ch = (a.n_out + a.group - 1) / a.group;
    a.region = ((f->n_num + 7) & ~7u) + a.group * f->factor + 8;   // lead-in (padded), the outputs' samples, the window's look-ahead word
    a.wide = ((uintptr_t)in_dev % 16 == 0 && (n_in * f->elem) % 16 == 0) ? 1u : 0u;
    HIP_LAUNCH(e, launch_filter_fir(f->is_q15(), a, e->stream));
    if (f->n_num > 1) f->cur ^= 1;
    f->count += n_in;
    return IQD_OK;
}

int iqd_filter_run(iqd_filter_t *f, const void *in, size_t n_in, void *out)
{
    int rc = filter_run_check(f, in, n_in, out, "iqd_filter_run");
    if (rc != IQD_OK) return rc;
    iqd_t *e = f->e;
    if (n_in == 0) return IQD_OK;
    (void)hipSetDevice(e->device);
    const size_t n_out = iqd_filter_out_count(f, n_in);
    const size_t ib = (size_t)f->n_ch * n_in * f->elem, ob = (size_t)f->n_ch * n_out * f->elem;
    HIP_TRY(e, f->st_in.ensure(ib));
    HIP_TRY(e, f->st_out.ensure(ob ? ob : 16));
    HIP_COPY(e, hipMemcpyAsync(f->st_in.p, in, ib, hipMemcpyHostToDevice, e->stream));
    rc = iqd_filter_run_device(f, f->st_in.p, n_in, f->st_out.p);
    if (rc != IQD_OK) return rc;
    if (ob) HIP_COPY(e, hipMemcpyAsync(out, f->st_out.p, ob, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

}  // extern "C"
