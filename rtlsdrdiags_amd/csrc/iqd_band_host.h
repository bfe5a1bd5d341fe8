// What the host code of the five band objects shares (iqd_spectrum.cpp, iqd_detect.cpp, iqd_track.cpp, iqd_measure.cpp,
// iqd_tracklog.cpp; the tone bank, iqd_tones.cpp, borrows BandArg, the create and reserved checks and destroy): one
// description of a call's pointer arguments, which drives the NULL refusals, the alignment refusals and the staged host call;
// the refusals with one text for all; destroy; and the tracker's and the log's state block.  A run refuses before it queues:
// NULLs in argument order, then the counts, then (run_device) the alignment.  Every text is ABI behaviour
// (tests/golden/band_refusals.json has each, and which wins).  No allocation per call.
#pragma once
#include "iqd_engine_impl.h"

namespace iqd {

// One pointer argument of run / run_device.  run_device reads name and ptr only.
struct BandArg {
    const char *name;    // as the messages spell it
    const void *ptr;     // the caller's array: on the host for run, on the device for run_device
    size_t bytes;        // of the whole array, for run's copies
    DevBuf *stage;       // where run keeps its device copy
    bool out;            // run copies it back, not in
};
template <size_t K> struct BandArgs { BandArg a[K]; };
constexpr bool BAND_IN = false, BAND_OUT = true;

constexpr uint32_t BAND_MIN_BINS = 64, BAND_MAX_BINS = 2048;
constexpr size_t BAND_MAX_ROWS = 0x7fffffffull;      // n_sources x n_blocks of one call

inline bool band_bins_ok(uint32_t n) { return n >= BAND_MIN_BINS && n <= BAND_MAX_BINS && (n & (n - 1)) == 0; }

// create's first refusals; without an engine there is nowhere to leave a text
inline int band_create_check(iqd_t *e, const void *cfg, const void *out, const char *who)
{
    if (!e) return IQD_EINVAL;
    if (!out) return e->fail(IQD_EINVAL, "%s: out is NULL", who);
    if (!cfg) return e->fail(IQD_EINVAL, "%s: cfg is NULL", who);
    return IQD_OK;
}

inline int band_bins_check(iqd_t *e, uint32_t n, const char *who)
{
    return band_bins_ok(n) ? IQD_OK : e->fail(IQD_EINVAL, "%s: n_bins (%u) must be 64, 128, 256, 512, 1024 or 2048", who, n);
}

template <int K> int band_reserved_check(iqd_t *e, const uint32_t (&reserved)[K], const char *who)
{
    for (int i = 0; i < K; i++)
        if (reserved[i]) return e->fail(IQD_EINVAL, "%s: reserved[%d] is not 0", who, i);
    return IQD_OK;
}

// what the object has queued on the engine's stream is done before its buffers go
template <class T> void band_destroy(T *o)
{
    if (!o) return;
    (void)hipSetDevice(o->e->device);
    (void)hipStreamSynchronize(o->e->stream);
    delete o;
}

template <size_t K> int band_null_check(iqd_t *e, const BandArgs<K> &args, const char *who)
{
    for (const BandArg &x : args.a)
        if (!x.ptr) return e->fail(IQD_EINVAL, "%s: %s is NULL", who, x.name);
    return IQD_OK;
}

// a run of n_blocks blocks of n_sources sources: the NULLs, then the count
template <size_t K> int band_run_check(iqd_t *e, const BandArgs<K> &args, size_t n_blocks, uint32_t n_sources, const char *who)
{
    int rc = band_null_check(e, args, who);
    if (rc != IQD_OK) return rc;
    if (n_blocks == 0) return e->fail(IQD_EINVAL, "%s: n_blocks is 0", who);
    if (n_blocks > BAND_MAX_ROWS / n_sources)
        return e->fail(IQD_EINVAL, "%s: n_blocks (%zu) times n_sources (%u) is more than one call covers (2^31 - 1)", who, n_blocks, n_sources);
    return IQD_OK;
}

template <size_t K> int band_align_check(iqd_t *e, const BandArgs<K> &args, const char *who)
{
    for (const BandArg &x : args.a)
        if ((uintptr_t)x.ptr % 16) return e->fail(IQD_EINVAL, "%s: %s_dev is not 16-byte aligned", who, x.name);
    return IQD_OK;
}

// The host form of a run whose args have passed its checks.  Every staging buffer is there before the first copy, so a failed
// allocation queues nothing; then the inputs go in, run_device() - the object's own, on the staging buffers - queues its
// launch, the outputs come back, and the call waits for them.
template <size_t K, class RunDevice> int band_staged_run(iqd_t *e, const BandArgs<K> &args, RunDevice run_device)
{
    (void)hipSetDevice(e->device);
    for (const BandArg &x : args.a) HIP_TRY(e, x.stage->ensure(x.bytes));
    for (const BandArg &x : args.a)
        if (!x.out) HIP_COPY(e, hipMemcpyAsync(x.stage->p, x.ptr, x.bytes, hipMemcpyHostToDevice, e->stream));
    int rc = run_device();
    if (rc != IQD_OK) return rc;
    for (const BandArg &x : args.a)
        if (x.out) HIP_COPY(e, hipMemcpyAsync(const_cast<void *>(x.ptr), x.stage->p, x.bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

// The tracker's and the log's state: [n_sources] rows of row_bytes (a source's S records), then [n_sources] tails of
// tail_bytes (its counter).
struct BandState {
    DevBuf buf;
    uint32_t n_sources = 0;
    size_t row_bytes = 0, tail_bytes = 0, bytes = 0;

    uint8_t *tails() const { return buf.as<uint8_t>() + n_sources * row_bytes; }

    int create(iqd_t *e, uint32_t sources, size_t row, size_t tail, const char *who)   // allocated and cleared
    {
        n_sources = sources; row_bytes = row; tail_bytes = tail; bytes = sources * (row + tail);
        (void)hipSetDevice(e->device);
        if (buf.ensure(bytes) != hipSuccess) return e->fail(IQD_ENOMEM, "%s: no device memory for %zu bytes of state", who, bytes);
        return reset(e);
    }

    int reset(iqd_t *e)   // one counted copy
    {
        (void)hipSetDevice(e->device);
        HIP_COPY(e, hipMemsetAsync(buf.p, 0, bytes, e->stream));
        return IQD_OK;
    }

    // get_state: a source's row, and its tail where the caller takes one; waits for them
    int read(iqd_t *e, uint32_t source, void *row_out, void *tail_out, const char *who)
    {
        if (source >= n_sources) return e->fail(IQD_EINVAL, "%s: source (%u) must be below n_sources (%u)", who, source, n_sources);
        (void)hipSetDevice(e->device);
        HIP_COPY(e, hipMemcpyAsync(row_out, buf.as<uint8_t>() + source * row_bytes, row_bytes, hipMemcpyDeviceToHost, e->stream));
        if (tail_out) HIP_COPY(e, hipMemcpyAsync(tail_out, tails() + source * tail_bytes, tail_bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(e, hipStreamSynchronize(e->stream));
        return IQD_OK;
    }
};

}  // namespace iqd
