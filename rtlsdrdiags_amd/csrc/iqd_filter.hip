// The reference's four hot-path filter classes as stand-alone, many-channel kernels (include/iqdemod.h: iqd_filter_*):
//   Decimator_int16::decimate / FirFilter_int16::filterData   filter_fir_kernel<int16_t>   (Q15, clamp after every MAC)
//   FirFilter::filterData                                      filter_fir_kernel<float>
//   IirFilter::filterData                                      filter_iir_small_kernel<NB, NA>, filter_iir_kernel
// Every sum runs in the reference's order; this translation unit is built with -ffp-contract=off like the rest.
//
// FIR: one lane per output.  A group of lanes (iqd_filter.h: 256, or 64 where rows are short, so that one workgroup then
// serves up to four channels) stages the samples behind its outputs from [history | this call] into LDS with coalesced
// loads (16 bytes per lane where every row is 16-byte aligned, one element per lane otherwise - the same values either
// way).  The taps are uniform: they are read through the scalar cache (constant address space), never per lane.  Q15:
// the taps [0, k0) cannot reach the clamp for any input (iqd_filter_clamp_free_taps), so they are summed two per
// v_dot2_i32_i16; from k0 on it is one multiply-add and one v_med3_i32 per tap, in order.  k0 = L never clamps.
// A second launch writes the history after the call.
//
// IIR: the recurrence is serial per channel and exact - one lane per channel, one wave per 64 channels, no scan.  Time is
// walked in tiles of 64 steps: the wave loads 64 rows x 64 steps coalesced along the rows into LDS (row pitch 65 floats),
// lane c then walks row c, overwriting x with y, and the tile goes out the way it came in.  Orders up to (3, 2) - both
// reference uses, any biquad - are instantiated with the state in registers; the general case keeps per-lane rings in
// LDS.  Fewer than 64 x (number of CUs) channels leave CUs idle; that is the price of the exact recurrence.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_filter.h"

namespace iqd {

// uniform, read-only for the kernel's lifetime: loads through this pointer type are scalar (s_load / the scalar cache)
typedef const uint32_t __attribute__((address_space(4))) *flt_cptr;

__device__ __forceinline__ flt_cptr flt_const(const void *p) { return (flt_cptr)(uintptr_t)p; }

__device__ __forceinline__ int flt_clamp_q30(int acc)   // folds to v_med3_i32
{
    const int lo = acc < -0x40000000 ? -0x40000000 : acc;
    return lo > 0x3fffffff ? 0x3fffffff : lo;
}

// acc + the two int16 products, no saturation (v_dot2_i32_i16; the tap word comes from a scalar register)
__device__ __forceinline__ int flt_dot2(uint32_t x, uint32_t h, int acc)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(x), "s"(h), "v"(acc));
    return r;
}

__device__ __forceinline__ float flt_u2f(uint32_t u) { return __builtin_bit_cast(float, u); }

// sample s of the channel's stream relative to this call's start: s < 0 is history (s >= -(L - 1)), s >= n_in reads 0
template <class T>
__device__ __forceinline__ T flt_sample(const FirLaunch &a, uint64_t ch, int64_t s)
{
    if (s >= (int64_t)a.n_in) return (T)0;
    if (s >= 0) return ((const T *)a.in)[ch * a.n_in + (uint64_t)s];
    const uint32_t h = a.n_taps - 1;
    return ((const T *)a.hist)[ch * h + (uint64_t)((int64_t)h + s)];
}

template <class T>
__global__ __launch_bounds__(FLT_WG) void filter_fir_kernel(const FirLaunch a)
{
    extern __shared__ uint4 flt_lds[];
    constexpr uint32_t E = 16 / sizeof(T);                  // elements per 16 bytes
    const uint32_t tid = threadIdx.x;
    const uint32_t sub = a.group == FLT_WG ? 0 : tid / FLT_WAVE;
    const uint32_t lane = a.group == FLT_WG ? tid : tid % FLT_WAVE;
    const uint64_t unit = (uint64_t)blockIdx.x * (FLT_WG / a.group) + sub;
    const uint64_t ch = unit / a.groups_per_ch;
    const uint32_t g = (uint32_t)(unit - ch * a.groups_per_ch);
    const bool live = ch < a.n_ch;                           // uniform over the group (a group is whole waves)
    T *reg = (T *)flt_lds + (size_t)sub * a.region;
    const uint32_t lead = a.n_taps - 1, lpad = (a.n_taps + 7) & ~7u;   // lpad > lead: the Q15 window may look one sample further back
    const uint32_t span = a.group * a.factor;               // samples this group's outputs consume
    const int64_t base = (int64_t)g * span;

    if (live) {
        for (uint32_t i = lane; i < lead; i += a.group)
            reg[lpad - lead + i] = flt_sample<T>(a, ch, base - (int64_t)lead + i);
        if (a.wide) {                                        // rows 16-byte aligned, n_in a multiple of E: whole chunks
            const uint4 *row = (const uint4 *)((const T *)a.in + ch * a.n_in);
            uint4 *dst = (uint4 *)(reg + lpad);
            for (uint32_t i = lane; i < span / E; i += a.group) {
                const uint64_t s = (uint64_t)base + (uint64_t)i * E;
                dst[i] = s < a.n_in ? row[s / E] : uint4{0, 0, 0, 0};
            }
        } else {
            for (uint32_t i = lane; i < span; i += a.group) reg[lpad + i] = flt_sample<T>(a, ch, base + i);
        }
    }
    __syncthreads();

    const uint64_t j = (uint64_t)g * a.group + lane;         // the lane's output in its row
    if (!live || j >= a.n_out) return;
    const uint32_t p = lpad + a.first + lane * a.factor;     // x[n] in the region; x[n - k] is at p - k
    const flt_cptr taps = flt_const(a.taps);
    if constexpr (sizeof(T) == 2) {
        // The taps come two per word, (h[k + 1], h[k]) in the (low, high) half, and meet (x[n - k - 1], x[n - k]): the
        // sample pair at m = p - 1 - k.  m keeps its parity over the even k, and half the lanes of an odd factor have it
        // odd - so every lane reads ALIGNED words, one per pair, and v_alignbit_b32 puts the pair together from the word
        // before and the word read last (shift 0 or 16 by the lane's parity).  An odd L ends on a zero tap.
        const uint32_t *W = (const uint32_t *)reg;
        const uint32_t m0 = p - 1, sh = (m0 & 1) * 16, wi = m0 >> 1, pairs = (a.n_taps + 1) >> 1, free_pairs = a.k0 >> 1;
        uint32_t hi = W[wi + 1], i = 0;
        int acc = 1 << 14;
        for (; i < free_pairs; i++) {                        // clamp-free prefix: two MACs per v_dot2_i32_i16
            const uint32_t lo = W[wi - i];
            acc = flt_dot2(__builtin_amdgcn_alignbit(hi, lo, sh), taps[i], acc);
            hi = lo;
        }
#pragma unroll 4
        for (; i < pairs; i++) {                             // from k0 on: one MAC and one v_med3_i32 per tap, in order
            const uint32_t lo = W[wi - i];
            const int xs = (int)__builtin_amdgcn_alignbit(hi, lo, sh), h = (int)taps[i];
            hi = lo;
            acc = flt_clamp_q30(acc + __mul24(h >> 16, xs >> 16));              // both factors are int16: the 24-bit multiply is exact
            acc = flt_clamp_q30(acc + __mul24((int)(short)h, (int)(short)xs));
        }
        ((int16_t *)a.out)[ch * a.n_out + j] = (int16_t)(acc >> 15);
    } else {
        float y = 0;
        const T *xp = reg + p;
        for (uint32_t k = 0; k < a.n_taps; k++) y = y + (flt_u2f(taps[k]) * xp[-(int)k]);
        ((float *)a.out)[ch * a.n_out + j] = y;
    }
}

// The history after the call: the last L - 1 samples of [history | input] (a call may be shorter than the history).
template <class T>
__global__ __launch_bounds__(FLT_WG) void filter_history_kernel(const FirLaunch a)
{
    const uint32_t h = a.n_taps - 1;
    const uint64_t t = (uint64_t)blockIdx.x * FLT_WG + threadIdx.x;
    if (t >= (uint64_t)a.n_ch * h) return;
    const uint64_t ch = t / h;
    const uint32_t k = (uint32_t)(t - ch * h);
    ((T *)a.hist_next)[t] = flt_sample<T>(a, ch, (int64_t)a.n_in - (int64_t)h + k);
}

// ---- IIR ------------------------------------------------------------------------------------------------------------
// tile[r][l] <- in[c0 + r][t0 + l] and back.  Narrow form: lane l moves column l of every row, 256 contiguous bytes per
// row and wave.  Wide form (every row 16-byte aligned, a whole tile): lane l moves four steps (l % 16) of the rows l / 16,
// l / 16 + 4, ..: a quarter of the memory instructions, the same values - and the loads of a whole tile are issued
// together, into registers, while the tile before is still being walked (iir_fetch, then iir_stash once the tile is free).
// Rows past the last channel are read from the last channel's row (valid memory) and never stored.
struct IirAhead { float4 v[FLT_WAVE / 4]; };

__device__ __forceinline__ bool iir_whole(const IirLaunch &a, uint32_t t0) { return a.wide && t0 < a.n_in && a.n_in - t0 >= FLT_IIR_TILE; }

__device__ __forceinline__ void iir_fetch(const IirLaunch &a, IirAhead &f, uint32_t c0, uint32_t rows, uint32_t t0, uint32_t lane)
{
    const uint32_t q = lane & 15, r0 = lane >> 4;
    const float *src = a.in + (size_t)c0 * a.n_in + t0 + 4 * q;
#pragma unroll
    for (uint32_t i = 0; i < FLT_WAVE / 4; i++) {
        const uint32_t r = r0 + 4 * i, rc = r < rows ? r : rows - 1;
        f.v[i] = *(const float4 *)(src + (size_t)rc * a.n_in);
    }
}

__device__ __forceinline__ void iir_stash(const IirAhead &f, float *tile, uint32_t lane)
{
    const uint32_t q = lane & 15, r0 = lane >> 4;
#pragma unroll
    for (uint32_t i = 0; i < FLT_WAVE / 4; i++) {
        float *d = tile + (r0 + 4 * i) * FLT_IIR_ROW + 4 * q;
        d[0] = f.v[i].x; d[1] = f.v[i].y; d[2] = f.v[i].z; d[3] = f.v[i].w;
    }
    __syncthreads();
}

__device__ __forceinline__ void iir_tile_in(const IirLaunch &a, float *tile, uint32_t c0, uint32_t rows, uint32_t t0, uint32_t nt,
                                            uint32_t lane)
{
    if (lane < nt) {
        const float *src = a.in + (size_t)c0 * a.n_in + t0 + lane;
#pragma unroll 4
        for (uint32_t r = 0; r < rows; r++) tile[r * FLT_IIR_ROW + lane] = src[(size_t)r * a.n_in];
    }
    __syncthreads();
}

__device__ __forceinline__ void iir_tile_out(const IirLaunch &a, const float *tile, uint32_t c0, uint32_t rows, uint32_t t0,
                                             uint32_t nt, uint32_t lane)
{
    __syncthreads();
    if (a.wide && nt == FLT_IIR_TILE) {
        const uint32_t q = lane & 15, r0 = lane >> 4;
        float *dst = a.out + (size_t)c0 * a.n_in + t0 + 4 * q;
#pragma unroll 4
        for (uint32_t i = 0; i < FLT_WAVE / 4; i++) {
            const uint32_t r = r0 + 4 * i;
            if (r < rows) {
                const float *d = tile + r * FLT_IIR_ROW + 4 * q;
                *(float4 *)(dst + (size_t)r * a.n_in) = float4{d[0], d[1], d[2], d[3]};
            }
        }
    } else if (lane < nt) {
        float *dst = a.out + (size_t)c0 * a.n_in + t0 + lane;
#pragma unroll 4
        for (uint32_t r = 0; r < rows; r++) dst[(size_t)r * a.n_in] = tile[r * FLT_IIR_ROW + lane];
    }
    __syncthreads();
}

// IirFilter::filterData, orders known at compile time: v = 0 + b0 x[n] + b1 x[n-1] + ..; r = 0 + a0 y[n-1] + ..; y = v - r
template <int NB, int NA>
__global__ __launch_bounds__(FLT_WAVE) void filter_iir_small_kernel(const IirLaunch a)
{
    __shared__ float tile[FLT_IIR_TILE * FLT_IIR_ROW];
    const uint32_t lane = threadIdx.x, c0 = blockIdx.x * FLT_WAVE, ch = c0 + lane;
    const uint32_t rows = a.n_ch - c0 < FLT_WAVE ? a.n_ch - c0 : FLT_WAVE;
    const bool live = lane < rows;
    const flt_cptr cf = flt_const(a.coef);
    float b[NB], d[NA], xs[NB], ys[NA];                      // xs[k] = x[n-k] (xs[0] is the step's input), ys[k] = y[n-1-k]
    for (int k = 0; k < NB; k++) b[k] = flt_u2f(cf[k]);
    for (int k = 0; k < NA; k++) d[k] = flt_u2f(cf[NB + k]);
    float *st = a.state + (size_t)ch * (NB - 1 + NA);
    for (int k = 1; k < NB; k++) xs[k] = live ? st[k - 1] : 0.f;
    for (int k = 0; k < NA; k++) ys[k] = live ? st[NB - 1 + k] : 0.f;

    IirAhead ahead;
    if (iir_whole(a, 0)) iir_fetch(a, ahead, c0, rows, 0, lane);
    for (uint32_t t0 = 0; t0 < a.n_in; t0 += FLT_IIR_TILE) {
        const uint32_t nt = a.n_in - t0 < FLT_IIR_TILE ? a.n_in - t0 : FLT_IIR_TILE;
        if (iir_whole(a, t0)) iir_stash(ahead, tile, lane);
        else iir_tile_in(a, tile, c0, rows, t0, nt, lane);
        if (iir_whole(a, t0 + FLT_IIR_TILE)) iir_fetch(a, ahead, c0, rows, t0 + FLT_IIR_TILE, lane);
        if (live) {
            float *row = tile + lane * FLT_IIR_ROW;
#pragma unroll 8
            for (uint32_t t = 0; t < nt; t++) {
                xs[0] = row[t];
                float v = 0, r = 0;
#pragma unroll
                for (int k = 0; k < NB; k++) v = v + (b[k] * xs[k]);
#pragma unroll
                for (int k = 0; k < NA; k++) r = r + (d[k] * ys[k]);
                const float y = v - r;
#pragma unroll
                for (int k = NB - 1; k > 0; k--) xs[k] = xs[k - 1];
#pragma unroll
                for (int k = NA - 1; k > 0; k--) ys[k] = ys[k - 1];
                ys[0] = y;
                row[t] = y;
            }
        }
        iir_tile_out(a, tile, c0, rows, t0, nt, lane);
    }
    if (live) {
        for (int k = 1; k < NB; k++) st[k - 1] = xs[k];
        for (int k = 0; k < NA; k++) st[NB - 1 + k] = ys[k];
    }
}

// Any order up to (64, 64): per-lane rings in LDS, ring[slot][lane]; the slots move uniformly, so the index arithmetic is scalar.
__global__ __launch_bounds__(FLT_WAVE) void filter_iir_kernel(const IirLaunch a)
{
    __shared__ float tile[FLT_IIR_TILE * FLT_IIR_ROW];
    __shared__ float xr[(FLT_IIR_MAX_ORDER - 1) * FLT_WAVE];   // past inputs
    __shared__ float yr[FLT_IIR_MAX_ORDER * FLT_WAVE];         // past outputs
    const uint32_t lane = threadIdx.x, c0 = blockIdx.x * FLT_WAVE, ch = c0 + lane;
    const uint32_t rows = a.n_ch - c0 < FLT_WAVE ? a.n_ch - c0 : FLT_WAVE;
    const bool live = lane < rows;
    const flt_cptr cf = flt_const(a.coef);
    const uint32_t nx = a.n_num - 1, ny = a.n_den;
    float *st = a.state + (size_t)ch * (nx + ny);
    // x[n-1-i] sits in slot (xh - i) mod nx, y[n-1-i] in slot (yh - i) mod ny
    uint32_t xh = nx ? nx - 1 : 0, yh = ny - 1;
    for (uint32_t i = 0; i < nx; i++) xr[(nx - 1 - i) * FLT_WAVE + lane] = live ? st[i] : 0.f;
    for (uint32_t i = 0; i < ny; i++) yr[(ny - 1 - i) * FLT_WAVE + lane] = live ? st[nx + i] : 0.f;

    IirAhead ahead;
    if (iir_whole(a, 0)) iir_fetch(a, ahead, c0, rows, 0, lane);
    for (uint32_t t0 = 0; t0 < a.n_in; t0 += FLT_IIR_TILE) {
        const uint32_t nt = a.n_in - t0 < FLT_IIR_TILE ? a.n_in - t0 : FLT_IIR_TILE;
        if (iir_whole(a, t0)) iir_stash(ahead, tile, lane);
        else iir_tile_in(a, tile, c0, rows, t0, nt, lane);
        if (iir_whole(a, t0 + FLT_IIR_TILE)) iir_fetch(a, ahead, c0, rows, t0 + FLT_IIR_TILE, lane);
        float *row = tile + lane * FLT_IIR_ROW;
        for (uint32_t t = 0; t < nt; t++) {
            const float x0 = row[t];
            float v = 0, r = 0;
            v = v + (flt_u2f(cf[0]) * x0);
            uint32_t s = xh;
            for (uint32_t k = 1; k <= nx; k++) {
                v = v + (flt_u2f(cf[k]) * xr[s * FLT_WAVE + lane]);
                s = s ? s - 1 : nx - 1;
            }
            s = yh;
            for (uint32_t k = 0; k < ny; k++) {
                r = r + (flt_u2f(cf[a.n_num + k]) * yr[s * FLT_WAVE + lane]);
                s = s ? s - 1 : ny - 1;
            }
            const float y = v - r;
            if (nx) {
                xh = xh + 1 == nx ? 0 : xh + 1;
                xr[xh * FLT_WAVE + lane] = x0;
            }
            yh = yh + 1 == ny ? 0 : yh + 1;
            yr[yh * FLT_WAVE + lane] = y;
            row[t] = y;
        }
        iir_tile_out(a, tile, c0, rows, t0, nt, lane);
    }
    if (live) {
        uint32_t s = xh;
        for (uint32_t i = 0; i < nx; i++) {
            st[i] = xr[s * FLT_WAVE + lane];
            s = s ? s - 1 : nx - 1;
        }
        s = yh;
        for (uint32_t i = 0; i < ny; i++) {
            st[nx + i] = yr[s * FLT_WAVE + lane];
            s = s ? s - 1 : ny - 1;
        }
    }
}

// ---- launch wrappers ------------------------------------------------------------------------------------------------
size_t fir_lds_bytes(const FirLaunch &a, bool q15)
{
    return (size_t)(FLT_WG / a.group) * a.region * (q15 ? 2 : 4);
}

hipError_t launch_filter_fir(bool q15, const FirLaunch &a, hipStream_t s)
{
    if (a.n_out) {
        const uint64_t units = (uint64_t)a.n_ch * a.groups_per_ch, per_wg = FLT_WG / a.group;
        const dim3 grid((unsigned)((units + per_wg - 1) / per_wg)), block(FLT_WG);
        const size_t lds = fir_lds_bytes(a, q15);
        if (q15) hipLaunchKernelGGL(filter_fir_kernel<int16_t>, grid, block, lds, s, a);
        else hipLaunchKernelGGL(filter_fir_kernel<float>, grid, block, lds, s, a);
    }
    const uint64_t nh = (uint64_t)a.n_ch * (a.n_taps - 1);
    if (nh) {
        const dim3 grid((unsigned)((nh + FLT_WG - 1) / FLT_WG)), block(FLT_WG);
        if (q15) hipLaunchKernelGGL(filter_history_kernel<int16_t>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(filter_history_kernel<float>, grid, block, 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_filter_iir(const IirLaunch &a, hipStream_t s)
{
    const dim3 grid((a.n_ch + FLT_WAVE - 1) / FLT_WAVE), block(FLT_WAVE);
    const uint32_t key = a.n_num <= 3 && a.n_den <= 2 ? a.n_num * 4 + a.n_den : 0;
    switch (key) {
    case 1 * 4 + 1: hipLaunchKernelGGL((filter_iir_small_kernel<1, 1>), grid, block, 0, s, a); break;
    case 1 * 4 + 2: hipLaunchKernelGGL((filter_iir_small_kernel<1, 2>), grid, block, 0, s, a); break;
    case 2 * 4 + 1: hipLaunchKernelGGL((filter_iir_small_kernel<2, 1>), grid, block, 0, s, a); break;
    case 2 * 4 + 2: hipLaunchKernelGGL((filter_iir_small_kernel<2, 2>), grid, block, 0, s, a); break;
    case 3 * 4 + 1: hipLaunchKernelGGL((filter_iir_small_kernel<3, 1>), grid, block, 0, s, a); break;
    case 3 * 4 + 2: hipLaunchKernelGGL((filter_iir_small_kernel<3, 2>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(filter_iir_kernel, grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

}  // namespace iqd
