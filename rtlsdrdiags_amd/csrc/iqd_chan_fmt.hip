// Wideband channelizer on signed captures (include/iqdemod.h: "Signed 8-bit and 16-bit captures"; IQD_WIDE_S8, IQD_WIDE_S16):
// chz_kernel's schedule (iqd_chan.hip) with the window staged as PLANES signed-byte planes, each of which looks exactly like
// chz_kernel's window, so that chz_b_operand and the A operands (chz_pack_rows' bytes) are used as they are.
//
//   S8   (PLANES = 1)  the plane is the capture's bytes as they are (no flip); the epilogue is chz_epilogue.
//   S16  (PLANES = 2)  sample x = 256 hi + lo' + 128 with hi = x >> 8 and lo' = (x & 255) - 128, both signed bytes: plane 0
//        holds hi, plane 1 lo', each I/Q interleaved, de-interleaved from the 4-byte samples while staging.  Per K-chunk
//        and 16-output tile the two tap planes meet the two sample planes (four MFMAs); the sums of each sample plane,
//        H = sum g hi and Lo' = sum g lo', are bounded like chz_kernel's A and fit int32.  With G the sum of the row's
//        coefficients (ChzFmtTile, from the host), A = 256 H + Lo, Lo = Lo' + 128 G, and by the nesting of floor divisions
//            (A + 2^15) >> 16 = (H + ((Lo + 2^15) >> 8)) >> 8.
//        Lo is formed in int64 (|Lo| <= 256 sum(|gr| + |gi|) can pass 2^31); (Lo + 2^15) >> 8 and its sum with H fit int32
//        again, and the value before sat16 is below 2^23, so that it enters chz_epilogue as a high tap plane with a zero low
//        one - (256 v + 128) >> 8 = v - and everything from sat16 on is chz_epilogue's own arithmetic.
//        An S16 step works on one 16-output tile where chz_kernel works on two: the same four accumulator chains.
//
// The history is raw capture bytes (the last Kp samples, 2 Kp B bytes per source; zero history is zero bytes) and goes
// through the same staging.  LDS is chz_kernel's: the planes share CHZ_WIN_MAX, so an S16 window covers half the outputs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan.h"
#include "iqd_chan_dev.h"

namespace iqd {

// Every thread of the workgroup: samples [M m0 - Kp, M (m0 + nloc)) of [history | this call] of one source into the
// PLANES planes at win + p * pstride.  A thread moves 16 plane bytes per plane and step (16 B capture bytes); the
// history's end and every step are aligned to that, so a step lies on one side of the boundary.
template <int PLANES>
__device__ __forceinline__ void chz_fmt_stage_window(const ChzFmtLaunch &f, uint32_t source, uint32_t m0, uint32_t nloc, uint8_t *win)
{
    const ChzLaunch &a = f.a;
    const uint32_t M = a.m, kp = a.kp;
    const size_t hb = (size_t)2 * kp * PLANES;                  // history bytes of one source
    const uint8_t *src = a.wide + (size_t)source * a.bytes_per_source;
    const uint8_t *hend = a.hist + (size_t)source * hb + hb;
    const int64_t s0 = (int64_t)m0 * M - (int64_t)kp;           // first sample of the window, a multiple of 32
    const uint32_t pbytes = 2 * (nloc * M + kp);                // bytes of one plane, a multiple of 64
    for (uint32_t i = threadIdx.x * 16; i < pbytes; i += blockDim.x * 16) {
        const int64_t b = (2 * s0 + i) * PLANES;                // capture byte of plane byte i
        const uint4 *p = (const uint4 *)(b < 0 ? hend + b : src + b);
        if (PLANES == 1) {
            *(uint4 *)(win + i) = p[0];
        } else {
            const uint4 u = p[0], v = p[1];                     // eight samples: (I lo, I hi, Q lo, Q hi) each
            uint4 hi, lo;
            hi.x = chz_fmt_hi(u.x, u.y); hi.y = chz_fmt_hi(u.z, u.w); hi.z = chz_fmt_hi(v.x, v.y); hi.w = chz_fmt_hi(v.z, v.w);
            lo.x = chz_fmt_lo(u.x, u.y); lo.y = chz_fmt_lo(u.z, u.w); lo.z = chz_fmt_lo(v.x, v.y); lo.w = chz_fmt_lo(v.z, v.w);
            *(uint4 *)(win + i) = hi;
            *(uint4 *)(win + f.pstride + i) = lo;
        }
    }
}

// chz_tile_outputs (iqd_chan.hip) for PLANES sample planes: NT = 2 / PLANES 16-output tiles at a time.
// acc[t][s][p]: tile t, sample plane s (S16: 0 = hi, 1 = lo'), tap plane p (0 = lo, 1 = hi).
template <int PLANES, int NQR>
__device__ __forceinline__ void chz_fmt_tile_outputs(const ChzFmtLaunch &f, const uint8_t *win, const uint32_t *sp, uint8_t *stage,
                                                     const chz_v4i (&A)[NQR > 0 ? NQR : 1][2], const uint4 *amat,
                                                     const uint32_t (&inc)[2], const uint32_t (&shv)[2], const int32_t (&rnd)[2],
                                                     const int32_t (&gs)[2][2], uint32_t st_ch, uint32_t m0, uint32_t nloc)
{
    constexpr int NT = 2 / PLANES;
    const ChzLaunch &a = f.a;
    const uint32_t lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const uint32_t st_cl = lane >> 3, st_piece = lane & 7;
    const uint32_t M = a.m, nq = a.nq;
    const chz_v4i zero = {0, 0, 0, 0};
    for (uint32_t grp = 0; grp * CHZ_GROUP < nloc; grp++) {
        const uint32_t ntl = min(4u, (nloc - grp * CHZ_GROUP) / 16);   // 2 or 4
        for (uint32_t tp = 0; tp < ntl; tp += NT) {
            chz_v4i acc[NT][PLANES][2];
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int s = 0; s < PLANES; s++) acc[t][s][0] = acc[t][s][1] = zero;
            const uint32_t obase = 2 * M * (grp * CHZ_GROUP + 16 * tp + col + 1) + 16 * g;
            if (NQR > 0) {
#pragma unroll
                for (int q = 0; q < NQR; q++)
                    if (q < (int)nq) {
#pragma unroll
                        for (int t = 0; t < NT; t++)
#pragma unroll
                            for (int s = 0; s < PLANES; s++) {
                                const chz_v4i b = chz_b_operand(win + s * f.pstride, obase + 2 * M * 16 * t + 64 * q);
                                acc[t][s][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[q][0], b, acc[t][s][0], 0, 0, 0);
                                acc[t][s][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[q][1], b, acc[t][s][1], 0, 0, 0);
                            }
                    }
            } else {
                for (uint32_t q = 0; q < nq; q++) {
                    const chz_v4i alo = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 0) * 64]);
                    const chz_v4i ahi = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 1) * 64]);
#pragma unroll
                    for (int t = 0; t < NT; t++)
#pragma unroll
                        for (int s = 0; s < PLANES; s++) {
                            const chz_v4i b = chz_b_operand(win + s * f.pstride, obase + 2 * M * 16 * t + 64 * q);
                            acc[t][s][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(alo, b, acc[t][s][0], 0, 0, 0);
                            acc[t][s][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ahi, b, acc[t][s][1], 0, 0, 0);
                        }
                }
            }
            // epilogue: lane (col, g) holds rows 4 g .. 4 g + 3 = channels 2 g, 2 g + 1 (re, im) of output col of each tile
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const uint32_t jt = 16 * (tp + t) + col;
                const uint32_t n32 = a.nbase + (m0 + grp * CHZ_GROUP + jt) * M + M - 1;   // mod 2^32
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const uint32_t p = sp[(n32 * inc[i]) >> 20];
                    uint32_t v;
                    if (PLANES == 1) {
                        v = chz_epilogue(acc[t][0][0][2 * i], acc[t][0][1][2 * i], acc[t][0][0][2 * i + 1], acc[t][0][1][2 * i + 1],
                                         p, rnd[i], shv[i]);
                    } else {
                        const int32_t vr = chz_fmt_stage_a(acc[t][0][0][2 * i], acc[t][0][1][2 * i], acc[t][PLANES - 1][0][2 * i],
                                                           acc[t][PLANES - 1][1][2 * i], gs[i][0]);
                        const int32_t vi = chz_fmt_stage_a(acc[t][0][0][2 * i + 1], acc[t][0][1][2 * i + 1],
                                                           acc[t][PLANES - 1][0][2 * i + 1], acc[t][PLANES - 1][1][2 * i + 1], gs[i][1]);
                        v = chz_epilogue(0, vr, 0, vi, p, rnd[i], shv[i]);   // (256 v + 128) >> 8 = v: sat16 and on
                    }
                    *(uint16_t *)(stage + (2 * g + i) * (2 * CHZ_GROUP) + 2 * jt) = (uint16_t)v;
                }
            }
        }
        chz_wave_fence();
        if (st_ch != CHZ_NONE && st_piece * 8 < ntl * 16) {
            const uint4 v = *(const uint4 *)(stage + st_cl * (2 * CHZ_GROUP) + 16 * st_piece);
            *(uint4 *)(a.out + (size_t)st_ch * a.out_row + 2 * (size_t)(m0 + grp * CHZ_GROUP) + 16 * st_piece) = v;
        }
        chz_wave_fence();
    }
}

template <int PLANES, int NQR>   // NQR > 0: nq <= NQR, the A operands stay in registers; 0: they are read per group
__global__ __launch_bounds__(512) void chz_fmt_kernel(const ChzFmtLaunch f)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t chz_lds[];
    const ChzLaunch &a = f.a;
    uint32_t *sp = (uint32_t *)chz_lds;
    uint8_t *stage_all = chz_lds + CHZ_PHASOR * 4;
    uint8_t *win = chz_lds + CHZ_LDS_FIXED;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const ChzWg w = a.wgs[blockIdx.y];
    const uint32_t m0 = blockIdx.x * a.t_blk;
    const uint32_t nloc = min(a.t_blk, a.n_out - m0);           // a multiple of 32
    const uint32_t nq = a.nq;

    for (uint32_t i = tid; i < CHZ_PHASOR / 4; i += blockDim.x) ((uint4 *)sp)[i] = ((const uint4 *)a.phasor)[i];
    chz_fmt_stage_window<PLANES>(f, w.source, m0, nloc, win);
    __syncthreads();
    if (wave >= w.n_tiles) return;

    const uint32_t tile = w.first_tile + wave;
    const ChzTile *T = a.tiles + tile;
    const uint32_t g = lane >> 4;
    uint32_t inc[2], shv[2];
    int32_t rnd[2], gs[2][2] = {{0, 0}, {0, 0}};
#pragma unroll
    for (int i = 0; i < 2; i++) {
        inc[i] = T->inc[2 * g + i];
        const uint32_t L = T->shift[2 * g + i];
        shv[i] = 22 - L;
        rnd[i] = 1 << (21 - L);
        if (PLANES == 2) {
            gs[i][0] = f.gsum[tile].g[2 * g + i][0];
            gs[i][1] = f.gsum[tile].g[2 * g + i][1];
        }
    }
    const uint32_t st_ch = T->ch[lane >> 3];
    uint8_t *stage = stage_all + wave * (CHZ_TILE_CH * 2 * CHZ_GROUP);
    const uint4 *amat = a.amat + (size_t)tile * nq * 2 * 64 + lane;

    chz_v4i A[NQR > 0 ? NQR : 1][2];
    if (NQR > 0) {
#pragma unroll
        for (int q = 0; q < NQR; q++)
            if (q < (int)nq) {
                A[q][0] = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 0) * 64]);
                A[q][1] = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 1) * 64]);
            }
    }
    chz_fmt_tile_outputs<PLANES, NQR>(f, win, sp, stage, A, amat, inc, shv, rnd, gs, st_ch, m0, nloc);
}

// the next call's history: the last 2 kp B raw bytes of [history | this call] per source
__global__ void chz_fmt_history_kernel(const ChzFmtLaunch f)
{
    const ChzLaunch &a = f.a;
    const uint32_t hb = 2 * a.kp * f.rail_bytes;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_sources * hb) return;
    const uint32_t s = t / hb, i = t - s * hb;
    const int64_t b = (int64_t)a.bytes_per_source - hb + i;
    a.hist_next[t] = b < 0 ? a.hist[(size_t)s * hb + hb + b] : a.wide[(size_t)s * a.bytes_per_source + b];
}

hipError_t launch_channelizer_fmt(const ChzFmtLaunch &f, uint32_t n_wgs, hipStream_t st)
{
    const ChzLaunch &a = f.a;
    if (f.rail_bytes != 1 && f.rail_bytes != 2) return hipErrorInvalidValue;
    const uint32_t planes = f.rail_bytes;
    const uint32_t pbytes = 2 * (a.t_blk * a.m + a.kp);
    if (f.pstride < pbytes + 16 || f.pstride % 16 != 0 || (size_t)planes * f.pstride > CHZ_WIN_MAX + 16 * planes)
        return hipErrorInvalidValue;                            // the planes and chz_b_operand's fifth dword stay in LDS
    const dim3 grid((a.n_out + a.t_blk - 1) / a.t_blk, n_wgs);
    const size_t lds = CHZ_LDS_FIXED + (size_t)planes * f.pstride;
    if (n_wgs) {
        const bool reg = a.nq <= CHZ_NQ_REG;
        if (planes == 1 && reg) hipLaunchKernelGGL((chz_fmt_kernel<1, CHZ_NQ_REG>), grid, dim3(512), lds, st, f);
        else if (planes == 1) hipLaunchKernelGGL((chz_fmt_kernel<1, 0>), grid, dim3(512), lds, st, f);
        else if (reg) hipLaunchKernelGGL((chz_fmt_kernel<2, CHZ_NQ_REG>), grid, dim3(512), lds, st, f);
        else hipLaunchKernelGGL((chz_fmt_kernel<2, 0>), grid, dim3(512), lds, st, f);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const uint32_t nh = a.n_sources * 2 * a.kp * f.rail_bytes;
    hipLaunchKernelGGL(chz_fmt_history_kernel, dim3((nh + 255) / 256), dim3(256), 0, st, f);
    return hipGetLastError();
}

}  // namespace iqd
