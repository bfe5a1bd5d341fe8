// What the host code of every object on the engine's stream shares - the five band objects (iqd_band_host.h has what is about
// bands) and the two PCM add-ons, iqd_tones.cpp and iqd_fsk.cpp (the PCM part, below): one description of a call's pointer
// arguments, which drives the NULL refusals, the alignment refusals and the staged host call; the create and reserved
// refusals with one text for all; destroy.  A run refuses before it queues: NULLs in argument order, then the counts, then
// (run_device) the alignment.  Every text is ABI behaviour (tests/golden/band_refusals.json has the band objects', and which
// wins).  No allocation per call.
#pragma once
#include "iqd_engine_impl.h"

namespace iqd {

// One pointer argument of run / run_device.  run_device reads name, ptr, align and optional only.
struct ObjArg {
    const char *name;        // as the messages spell it
    const void *ptr;         // the caller's array: on the host for run, on the device for run_device
    size_t bytes;            // of the whole array, for run's copies
    DevBuf *stage;           // where run keeps its device copy
    bool out;                // run copies it back, not in
    uint32_t align = 16;     // what run_device asks of the address
    bool optional = false;   // the caller may leave it out (NULL): then not refused, not staged, not copied

    bool left_out() const { return optional && !ptr; }
};
template <size_t K> struct ObjArgs { ObjArg a[K]; };
constexpr bool ARG_IN = false, ARG_OUT = true, ARG_OPTIONAL = true;

// create's first refusals; without an engine there is nowhere to leave a text
inline int obj_create_check(iqd_t *e, const void *cfg, const void *out, const char *who)
{
    if (!e) return IQD_EINVAL;
    if (!out) return e->fail(IQD_EINVAL, "%s: out is NULL", who);
    if (!cfg) return e->fail(IQD_EINVAL, "%s: cfg is NULL", who);
    return IQD_OK;
}

template <int K> int obj_reserved_check(iqd_t *e, const uint32_t (&reserved)[K], const char *who)
{
    for (int i = 0; i < K; i++)
        if (reserved[i]) return e->fail(IQD_EINVAL, "%s: reserved[%d] is not 0", who, i);
    return IQD_OK;
}

// what the object has queued on the engine's stream is done before its buffers go
template <class T> void obj_destroy(T *o)
{
    if (!o) return;
    (void)hipSetDevice(o->e->device);
    (void)hipStreamSynchronize(o->e->stream);
    delete o;
}

template <size_t K> int obj_null_check(iqd_t *e, const ObjArgs<K> &args, const char *who)
{
    for (const ObjArg &x : args.a)
        if (!x.ptr && !x.optional) return e->fail(IQD_EINVAL, "%s: %s is NULL", who, x.name);
    return IQD_OK;
}

template <size_t K> int obj_align_check(iqd_t *e, const ObjArgs<K> &args, const char *who)
{
    for (const ObjArg &x : args.a)
        if ((uintptr_t)x.ptr % x.align) return e->fail(IQD_EINVAL, "%s: %s_dev is not %u-byte aligned", who, x.name, x.align);
    return IQD_OK;
}

// The host form of a run whose args have passed its checks; an array the caller left out is skipped throughout.  Every staging
// buffer is there before the first copy, so a failed allocation queues nothing (an empty array's too: run_device gets a pointer,
// no copy is made); then the inputs go in, run_device() - the object's own, on the staging buffers - queues its launches, the
// outputs come back, and the call waits for them.
template <size_t K, class RunDevice> int obj_staged_run(iqd_t *e, const ObjArgs<K> &args, RunDevice run_device)
{
    (void)hipSetDevice(e->device);
    for (const ObjArg &x : args.a)
        if (!x.left_out()) HIP_TRY(e, x.stage->ensure(std::max<size_t>(x.bytes, 16)));
    for (const ObjArg &x : args.a)
        if (!x.left_out() && !x.out && x.bytes) HIP_COPY(e, hipMemcpyAsync(x.stage->p, x.ptr, x.bytes, hipMemcpyHostToDevice, e->stream));
    int rc = run_device();
    if (rc != IQD_OK) return rc;
    for (const ObjArg &x : args.a)
        if (!x.left_out() && x.out && x.bytes) HIP_COPY(e, hipMemcpyAsync(const_cast<void *>(x.ptr), x.stage->p, x.bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

// ---- the PCM add-ons: objects that read [n_channels][row_stride] int16 rows, the first n samples of each ------------------------

constexpr size_t PCM_MAX_N = 0x7fffffffull;   // of n and row_stride (the kernels' TON_MAX_N and FSK_MAX_N)

// create's refusals up to the channel count
template <class Config> int pcm_create_check(iqd_t *e, const Config *cfg, const void *out, uint32_t abi_version, const char *who)
{
    int rc = obj_create_check(e, cfg, out, who);
    if (rc != IQD_OK) return rc;
    if (cfg->abi_version != abi_version) return e->fail(IQD_EINVAL, "%s: abi_version (%u) must be %u", who, cfg->abi_version, abi_version);
    if (cfg->n_channels == 0 || cfg->n_channels > (1u << 20))
        return e->fail(IQD_EINVAL, "%s: n_channels (%u) must be 1 .. 2^20", who, cfg->n_channels);
    return IQD_OK;
}

// run's and run_device's refusals up to the counts: another engine's object (the text is left with the object's engine), the
// NULLs in argument order, then n and row_stride
template <size_t K> int pcm_run_check(iqd_t *e, iqd_t *owner, const ObjArgs<K> &args, size_t row_stride, size_t n, const char *who)
{
    if (e != owner) return owner->fail(IQD_EINVAL, "%s: t belongs to another engine", who);
    int rc = obj_null_check(e, args, who);
    if (rc != IQD_OK) return rc;
    if (n > row_stride) return e->fail(IQD_EINVAL, "%s: n (%zu) is more than row_stride (%zu)", who, n, row_stride);
    if (row_stride > PCM_MAX_N) return e->fail(IQD_EINVAL, "%s: row_stride (%zu) is more than 2^31 - 1", who, row_stride);
    return IQD_OK;
}

// get_state: one channel's record of the [n_channels] on the device; waits for it
template <class State>
int pcm_get_state(iqd_t *e, const State *states, uint32_t n_channels, uint32_t channel, void *state, const char *who)
{
    if (!state) return e->fail(IQD_EINVAL, "%s: state is NULL", who);
    if (channel >= n_channels) return e->fail(IQD_EINVAL, "%s: channel (%u) must be below n_channels (%u)", who, channel, n_channels);
    (void)hipSetDevice(e->device);
    HIP_COPY(e, hipMemcpyAsync(state, states + channel, sizeof(State), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

// a tone's (or a bit clock's) phase increment: 2^32 freq / rate rounded to nearest, freq in thousandths
inline int pcm_phase_inc(uint64_t freq_mhz, uint32_t rate_hz, uint32_t *d)
{
    if (!d || rate_hz == 0 || freq_mhz >= 500ull * rate_hz) return IQD_EINVAL;
    const unsigned __int128 num = ((unsigned __int128)freq_mhz << 32) + 500ull * rate_hz;
    *d = (uint32_t)(num / (1000ull * rate_hz));
    return IQD_OK;
}

}  // namespace iqd
