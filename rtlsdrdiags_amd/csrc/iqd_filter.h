// The stand-alone filter classes (include/iqdemod.h: iqd_filter_*): what iqd_filter.cpp and iqd_filter.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace iqd {

// FIR kinds: a workgroup is FLT_WG lanes, one output each.  The lanes form groups of FLT_WG (long rows: one group, one
// channel) or FLT_WAVE lanes (rows of fewer than FLT_WG outputs: four groups, which may be four channels); a group stages
// the samples behind its outputs, [lead-in of L - 1 | group outputs x factor], in its own part of LDS.
constexpr uint32_t FLT_WG = 256, FLT_WAVE = 64;
constexpr uint32_t FLT_MAX_TAPS = 1024, FLT_MAX_FACTOR = 64;
// IIR: one lane per channel, one wave (one workgroup) per 64 channels, time in tiles of FLT_IIR_TILE steps
constexpr uint32_t FLT_IIR_TILE = 64, FLT_IIR_MAX_ORDER = 64;
constexpr uint32_t FLT_IIR_ROW = FLT_IIR_TILE + 1;   // LDS row pitch in floats: lane c walks row c without bank conflicts

struct FirLaunch {
    const void *in;        // [n_ch][n_in]
    void *out;             // [n_ch][n_out]
    const void *hist;      // [n_ch][n_taps - 1]: the samples before this call, oldest first (zeros at the stream start)
    void *hist_next;       // the same after this call
    // Q15: [ceil(L / 2) words: taps (2i + 1, 2i) in the (low, high) half, an odd L ending on a zero tap]; float: [L floats]
    const uint32_t *taps;
    uint32_t n_ch, n_in, n_out, n_taps, factor, first;   // first: input index of this call's first output
    uint32_t k0;           // Q15: taps [0, k0) are summed with dot2 and no clamp (k0 even), the rest one by one
    uint32_t group;        // lanes per group: FLT_WG or FLT_WAVE
    uint32_t groups_per_ch, region;   // region: samples of LDS per group
    uint32_t wide;         // every row of `in` is 16-byte aligned: stage with 16-byte loads
};

struct IirLaunch {
    const float *in;       // [n_ch][n_in]
    float *out;            // [n_ch][n_in]
    float *state;          // [n_ch][n_num - 1 + n_den]: x[n-1] .. x[n-n_num+1], y[n-1] .. y[n-n_den]
    const float *coef;     // [n_num + n_den]
    uint32_t n_ch, n_in, n_num, n_den;
    uint32_t wide;         // every row of `in` and `out` is 16-byte aligned: whole tiles move 16 bytes per lane
};

size_t fir_lds_bytes(const FirLaunch &a, bool q15);
hipError_t launch_filter_fir(bool q15, const FirLaunch &a, hipStream_t s);
hipError_t launch_filter_iir(const IirLaunch &a, hipStream_t s);

}  // namespace iqd
