// What the host code of the five band objects shares beyond iqd_obj_host.h (iqd_spectrum.cpp, iqd_detect.cpp, iqd_track.cpp,
// iqd_measure.cpp, iqd_tracklog.cpp): the bin counts and their refusal, a run's NULL and block-count refusals, and the tracker's
// and the log's state block.  Every text is ABI behaviour (tests/golden/band_refusals.json has each, and which wins).
#pragma once
#include "iqd_obj_host.h"

namespace iqd {

constexpr uint32_t BAND_MIN_BINS = 64, BAND_MAX_BINS = 2048;
constexpr size_t BAND_MAX_ROWS = 0x7fffffffull;      // n_sources x n_blocks of one call

inline bool band_bins_ok(uint32_t n) { return n >= BAND_MIN_BINS && n <= BAND_MAX_BINS && (n & (n - 1)) == 0; }

inline int band_bins_check(iqd_t *e, uint32_t n, const char *who)
{
    return band_bins_ok(n) ? IQD_OK : e->fail(IQD_EINVAL, "%s: n_bins (%u) must be 64, 128, 256, 512, 1024 or 2048", who, n);
}

// a run of n_blocks blocks of n_sources sources: the NULLs, then the count
template <size_t K> int band_run_check(iqd_t *e, const ObjArgs<K> &args, size_t n_blocks, uint32_t n_sources, const char *who)
{
    int rc = obj_null_check(e, args, who);
    if (rc != IQD_OK) return rc;
    if (n_blocks == 0) return e->fail(IQD_EINVAL, "%s: n_blocks is 0", who);
    if (n_blocks > BAND_MAX_ROWS / n_sources)
        return e->fail(IQD_EINVAL, "%s: n_blocks (%zu) times n_sources (%u) is more than one call covers (2^31 - 1)", who, n_blocks, n_sources);
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
