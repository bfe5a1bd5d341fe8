// PCM tone bank (include/iqdemod_tones.h; what the host passes: iqd_tones.h).  Two launches per call, whatever n and the
// number of frames are.
//
// ton_frames_kernel   a workgroup of four waves owns 16 channels x one frame slot f (the slots past 65535 / the grid's limit
//                     by a stride loop).  Per frame it is a GEMM [2 T x L] coefficients times [L x 16] samples on
//                     v_mfma_i32_16x16x64_i8.  Both operands are 16-bit, v = 256 hi + lo' + 128 with hi = v >> 8 and
//                     lo' = (v & 255) - 128 both signed bytes, so
//                         sum c x = 65536 S(ch, xh) + 256 (S(ch, xl') + S(cl', xh)) + S(cl', xl') + 128 sum c + 128 sum x - 16384 L
//                     with three int32 accumulators per result (|S| <= 2^27, the middle one 2^28, at L = 8192), sum c from
//                     the host (TonLaunch::gsum) and sum x formed while staging.
//     staging         TON_KC samples of the 16 channels at a time into two byte planes in LDS (a row per channel, 16 bytes of
//                     padding per row so that the 16 rows of a ds_read_b128 start in different banks): thread (col, sub)
//                     takes four consecutive samples of channel col from 4 sub on, every 64 - 2-byte loads, the rows need no
//                     more alignment - from the carried open frame below `fill` (slot 0 only) and from the call's row above;
//                     it sums x and x^2 on the way.  Samples of the padding (L = 32, 96: up to the 64 of a K-chunk) and of
//                     channels that do not complete slot f are zero bytes; the A operands are zero there too.
//     MFMA            wave w runs row tiles w and w + 4 (8 tones each: row 2 t' = c, 2 t' + 1 = s): per 64-sample K-chunk two
//                     16-byte A loads (global, the same for every workgroup: L2), two B reads, four MFMAs.
//                     Operand maps as iqd_chan_layout.cpp packs them: lane (r, g) holds A[row r][k = 16 g + j] and
//                     B[k = 16 g + j][col r]; the result's lane (col, g) holds rows 4 g .. 4 g + 3 of column col: Ar, Ai of
//                     tones 2 g and 2 g + 1 of the tile.
//     epilogue        the rounding, p = ar^2 + ai^2 into LDS [16][T]; then thread col walks its channel's T powers for best
//                     and second, decides the hit with 128-bit products in two halves, and stores the record with
//                     tone = f (the hit's tone or -1) and flags = 0; 16 threads per channel store the power row.
//                     A channel that does not complete slot f gets zero bytes.
// ton_close_kernel    one wave per channel: lane 0 walks the channel's k records in order through the decision recurrence
//                     (tone and flags rewritten in place), stores the count and the state; the 64 lanes move the samples
//                     behind the last whole frame into the open frame.
// No atomics, nothing to zero beforehand; the result cannot depend on the launch shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_tones.h"

namespace iqd {

typedef int ton_v4i __attribute__((ext_vector_type(4)));

constexpr uint32_t TON_PLANE_STRIDE = TON_KC + 16;

__device__ __forceinline__ uint32_t ton_count(const TonLaunch &a, uint32_t ch) { return a.count ? min(a.count[ch], a.n) : a.n; }

// 256 a >= b c in 128 bits
__device__ __forceinline__ bool ton_ge(uint64_t a, uint64_t b, uint64_t c)
{
    const uint64_t lh = a >> 56, ll = a << 8, rh = __umul64hi(b, c), rl = b * c;
    return lh > rh || (lh == rh && ll >= rl);
}

struct TonShared {
    uint8_t b[2][TON_TILE_CH][TON_PLANE_STRIDE];
    uint64_t p[TON_TILE_CH][TON_MAX_T];
    uint64_t e[TON_TILE_CH];
    int32_t sx[TON_TILE_CH];
    uint32_t fill[TON_TILE_CH], act[TON_TILE_CH];
};

__device__ __forceinline__ void ton_frame(const TonLaunch &a, TonShared &s, uint32_t f, uint32_t ch0)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t L = a.L, T = a.T, Lp = ton_padded(L), NQ = Lp / 64, NT = ton_row_tiles(T);

    if (tid < TON_TILE_CH) {
        const uint32_t ch = ch0 + tid;
        uint32_t fill = 0, act = 0;
        if (ch < a.n_channels) {
            fill = a.state[ch].fill;
            act = f < (fill + ton_count(a, ch)) / L;
        }
        s.fill[tid] = fill;
        s.act[tid] = act;
    }
    __syncthreads();
    uint32_t any = 0;
    for (uint32_t i = 0; i < TON_TILE_CH; i++) any |= s.act[i];

    const uint32_t col = tid >> 4, sub = tid & 15, ch = ch0 + col;
    const bool act = s.act[col] != 0;

    if (any) {
        const uint32_t fill = s.fill[col];
        const int16_t *row = a.pcm + (size_t)ch * a.row_stride;       // read for active channels only: ch < n_channels
        const int16_t *op = a.open + (size_t)ch * L;
        const int64_t off = (int64_t)f * L - fill;                     // frame sample k is row[off + k] from k = fill (f = 0) on
        int32_t sx = 0;
        uint64_t se = 0;
        ton_v4i acc[2][3];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) acc[i][j] = ton_v4i{0, 0, 0, 0};

        for (uint32_t kc0 = 0; kc0 < Lp; kc0 += TON_KC) {
            const uint32_t kcn = min(TON_KC, Lp - kc0);
            for (uint32_t k4 = sub * 4; k4 < kcn; k4 += 64) {
                uint32_t hi = 0, lo = 0;
                if (act) {
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) {
                        const uint32_t k = kc0 + k4 + j;
                        if (k < L) {
                            const int32_t x = f == 0 && k < fill ? op[k] : row[off + k];
                            sx += x;
                            se += (uint64_t)(uint32_t)(x * x);
                            hi |= (((uint32_t)x >> 8) & 255u) << (8 * j);
                            lo |= (((uint32_t)x & 255u) ^ 128u) << (8 * j);
                        }
                    }
                }
                *(uint32_t *)&s.b[0][col][k4] = hi;
                *(uint32_t *)&s.b[1][col][k4] = lo;
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const uint32_t rt = wave + TON_WAVES * i;
                if (rt < NT) {
                    const uint4 *am = a.amat + ((size_t)rt * NQ + kc0 / 64) * 2 * 64 + lane;
                    const uint8_t *bh = &s.b[0][lane & 15][16 * (lane >> 4)], *bl = &s.b[1][lane & 15][16 * (lane >> 4)];
                    for (uint32_t q = 0; q < kcn / 64; q++) {
                        const ton_v4i ah = __builtin_bit_cast(ton_v4i, am[(q * 2 + 0) * 64]);
                        const ton_v4i al = __builtin_bit_cast(ton_v4i, am[(q * 2 + 1) * 64]);
                        const ton_v4i xh = __builtin_bit_cast(ton_v4i, *(const uint4 *)(bh + 64 * q));
                        const ton_v4i xl = __builtin_bit_cast(ton_v4i, *(const uint4 *)(bl + 64 * q));
                        acc[i][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, xh, acc[i][0], 0, 0, 0);
                        acc[i][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, xl, acc[i][1], 0, 0, 0);
                        acc[i][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, xh, acc[i][1], 0, 0, 0);
                        acc[i][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, xl, acc[i][2], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }

        // a channel's sums over its 16 threads (consecutive lanes of one wave)
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            sx += __shfl_xor(sx, d);
            se += (uint64_t)__shfl_xor((unsigned long long)se, d);
        }
        if (sub == 0) { s.sx[col] = sx; s.e[col] = se; }
        __syncthreads();

        const uint32_t c = lane & 15, g = lane >> 4;
        const int64_t fixed = 128 * (int64_t)s.sx[c] - 16384 * (int64_t)L;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint32_t rt = wave + TON_WAVES * i;
            if (rt < NT) {
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const uint32_t t = rt * 8 + 2 * g + j, r = rt * TON_TILE_ROWS + 4 * g + 2 * j;
                    int64_t v[2];
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const int64_t A = 65536 * (int64_t)acc[i][0][2 * j + h] + 256 * (int64_t)acc[i][1][2 * j + h] +
                                          (int64_t)acc[i][2][2 * j + h] + 128 * (int64_t)a.gsum[r + h] + fixed;
                        v[h] = (A + 32768) >> 16;
                    }
                    if (t < T) s.p[c][t] = (uint64_t)(v[0] * v[0]) + (uint64_t)(v[1] * v[1]);
                }
            }
        }
        __syncthreads();
    }

    if (ch < a.n_channels && a.power) {
        uint64_t *pw = a.power + ((size_t)ch * a.F + f) * T;
        for (uint32_t t = sub; t < T; t += 16) pw[t] = act ? s.p[col][t] : 0;
    }
    if (tid < TON_TILE_CH && ch0 + tid < a.n_channels) {
        uint64_t r[5] = {0, 0, 0, 0, 0};
        if (s.act[tid]) {
            const uint64_t *p = s.p[tid];
            uint32_t best = 0, second = 0xffffffffu;
            uint64_t pb = p[0], ps = 0;
            for (uint32_t t = 1; t < T; t++) {
                const uint64_t v = p[t];
                if (v > pb) { second = best; ps = pb; best = t; pb = v; }
                else if (second == 0xffffffffu || v > ps) { second = t; ps = v; }
            }
            const uint64_t E = s.e[tid];
            const bool hit = pb >= a.min_power && ton_ge(pb, a.ratio_q8, ps) && ton_ge(pb, a.energy_q8, E);
            r[0] = E; r[1] = pb; r[2] = ps;
            r[3] = (uint64_t)best | (uint64_t)second << 32;
            r[4] = hit ? best : 0xffffffffu;
        }
        uint64_t *out = a.frames + ((size_t)(ch0 + tid) * a.F + f) * 5;
#pragma unroll
        for (int i = 0; i < 5; i++) out[i] = r[i];
    }
    __syncthreads();   // the next slot reuses s
}

__global__ __launch_bounds__(TON_WAVES * 64) void ton_frames_kernel(const TonLaunch a)
{
    __shared__ __attribute__((aligned(16))) TonShared s;
    for (uint32_t f = blockIdx.y; f < a.F; f += gridDim.y) ton_frame(a, s, f, blockIdx.x * TON_TILE_CH);
}

__global__ __launch_bounds__(64) void ton_close_kernel(const TonLaunch a)
{
    const uint32_t ch = blockIdx.x, lane = threadIdx.x, L = a.L;
    const TonState st = a.state[ch];
    const uint32_t m = ton_count(a, ch), k = (st.fill + m) / L;

    // the open frame: behind what it holds if no frame was completed, else anew from the sample behind the last whole frame
    const uint32_t left = st.fill + m - k * L;
    const uint32_t dst0 = k ? 0 : st.fill, cnt = k ? left : m;
    const int16_t *src = a.pcm + (size_t)ch * a.row_stride + (k ? (size_t)k * L - st.fill : 0);
    int16_t *dst = a.open + (size_t)ch * L + dst0;
    for (uint32_t i = lane; i < cnt; i += 64) dst[i] = src[i];

    if (lane != 0) return;
    int32_t tone = st.tone, cand = st.cand;
    uint32_t run = st.run, miss = st.miss;
    uint64_t *rec = a.frames + (size_t)ch * a.F * 5 + 4;
    for (uint32_t j = 0; j < k; j++, rec += 5) {
        const int32_t f = (int32_t)(uint32_t)rec[0];
        uint32_t flags = 0;
        if (f >= 0 && f == cand) run += run != 0xffffffffu;
        else { cand = f; run = f >= 0; }
        if (tone >= 0) {
            if (f == tone) miss = 0; else miss++;
            if (miss > a.hold) { tone = -1; miss = 0; flags |= 2u; }
        }
        if (tone < 0 && cand >= 0 && run >= a.open_frames) { tone = cand; miss = 0; flags |= 1u; }
        rec[0] = (uint64_t)(uint32_t)tone | (uint64_t)flags << 32;
    }
    TonState o{};
    o.tone = tone; o.cand = cand; o.run = run; o.miss = miss; o.fill = left;
    a.state[ch] = o;
    a.n_frames[ch] = k;
}

__global__ void ton_reset_kernel(TonState *state, uint32_t n_channels)
{
    const uint32_t ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= n_channels) return;
    TonState o{};
    o.tone = o.cand = -1;
    state[ch] = o;
}

hipError_t launch_tones_reset(TonState *state, uint32_t n_channels, hipStream_t s)
{
    if (!state || n_channels == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ton_reset_kernel, dim3((n_channels + 255) / 256), dim3(256), 0, s, state, n_channels);
    return hipGetLastError();
}

static bool ton_launch_ok(const TonLaunch &a)
{
    return a.n_channels >= 1 && a.n_channels <= (1u << 20) && a.L >= TON_MIN_L && a.L <= TON_MAX_L && a.L % 32 == 0 && a.T >= 1 &&
           a.T <= TON_MAX_T && a.n <= TON_MAX_N && a.row_stride <= TON_MAX_N && a.n <= a.row_stride && a.F == (a.n + a.L - 1) / a.L;
}

hipError_t launch_tones_frames(const TonLaunch &a, hipStream_t s)
{
    if (!ton_launch_ok(a) || a.F == 0) return hipErrorInvalidValue;
    const uint32_t gx = (a.n_channels + TON_TILE_CH - 1) / TON_TILE_CH;
    const uint32_t gy = min(a.F, min(65535u, (1u << 23) / gx));   // below 2^32 threads in all; the other slots by the stride loop
    hipLaunchKernelGGL(ton_frames_kernel, dim3(gx, gy), dim3(TON_WAVES * 64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_tones_close(const TonLaunch &a, hipStream_t s)
{
    if (!ton_launch_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ton_close_kernel, dim3(a.n_channels), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace iqd
