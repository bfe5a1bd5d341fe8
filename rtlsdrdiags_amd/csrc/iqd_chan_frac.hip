// Wideband channelizer at a fractional decimation P / Q, Q = 2, 4, 8 (include/iqdemod.h: "Fractional decimation"; layout of
// the operands: iqd_chan.h).  A decimator by P / Q is Q interleaved integer decimators by P with different tap sets: the
// outputs m = rho + Q t of residue rho use branch ((rho + 1) P - 1) mod Q at n = P t + floor(((rho + 1) P - 1) / Q).  Grid,
// window staging, MFMA / epilogue / 16-byte stores as chz_kernel (iqd_chan.hip); what differs: the 16 columns of one MFMA
// are 16 outputs of ONE residue (window stride 2 P bytes), its A operand is that residue's tap set, read per group, and a
// store group is 16 max(4, Q) consecutive outputs assembled from the Q residues in the wave's staging row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan.h"
#include "iqd_chan_dev.h"

namespace iqd {

// Fractional decimation P / Q (iqd_chan.h): one wave, its tile's outputs [m0, m0 + nloc) - whole store groups of G =
// chz_frac_group(Q) outputs, m0 a multiple of G - from the window staged for the wide samples of t0 = m0 / Q on.  MFMA
// tile ti of a group is residue rho = ti % Q, 16 outputs rho + Q (16 (ti / Q) + col): an integer decimator by P whose
// windows start at byte 2 (P t + e_rho + 1), e_rho = ((rho + 1) P - 1) / Q.  The A operands of the residues are read per
// group (Q sets of nq chunks do not stay in registers); two tiles at a time, four independent accumulator chains.
template <int Q>
__device__ __forceinline__ void chz_frac_tile_outputs(const ChzLaunch &a, const uint8_t *win, const uint32_t *sp, uint8_t *stage,
                                                      const uint4 *amat, const uint32_t (&inc)[2], const uint32_t (&shv)[2],
                                                      const int32_t (&rnd)[2], uint32_t st_ch, uint32_t m0, uint32_t nloc)
{
    constexpr uint32_t G = chz_frac_group(Q), NT = G / 16, TG = G / Q;   // outputs, MFMA tiles, wide steps t per group
    const uint32_t lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const uint32_t st_cl = lane >> 3, st_piece = lane & 7;
    const uint32_t P = a.m, nq = a.nq;
    const uint32_t t0 = m0 / Q;
    const chz_v4i zero = {0, 0, 0, 0};
    for (uint32_t grp = 0; grp * G < nloc; grp++) {
#pragma unroll
        for (uint32_t tp = 0; tp < NT; tp += 2) {
            chz_v4i acc[2][2] = {{zero, zero}, {zero, zero}};
            uint32_t e[2], tt[2], ob[2];
            const uint4 *am[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const uint32_t rho = (tp + t) % Q;
                e[t] = ((rho + 1) * P - 1) / Q;
                tt[t] = grp * TG + 16 * ((tp + t) / Q) + col;            // wide step within the window
                ob[t] = 2 * (P * tt[t] + e[t] + 1) + 16 * g;
                am[t] = amat + (size_t)rho * nq * 2 * 64;
            }
            for (uint32_t q = 0; q < nq; q++) {
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const chz_v4i alo = __builtin_bit_cast(chz_v4i, am[t][(q * 2 + 0) * 64]);
                    const chz_v4i ahi = __builtin_bit_cast(chz_v4i, am[t][(q * 2 + 1) * 64]);
                    const chz_v4i b = chz_b_operand(win, ob[t] + 64 * q);
                    acc[t][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(alo, b, acc[t][0], 0, 0, 0);
                    acc[t][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ahi, b, acc[t][1], 0, 0, 0);
                }
            }
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const uint32_t rho = (tp + t) % Q;
                const uint32_t jt = rho + Q * (16 * ((tp + t) / Q) + col);   // output within the group
                const uint32_t n32 = a.nbase + (t0 + tt[t]) * P + e[t];      // mod 2^32
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const uint32_t p = sp[(n32 * inc[i]) >> 20];
                    const uint32_t v = chz_epilogue(acc[t][0][2 * i], acc[t][1][2 * i], acc[t][0][2 * i + 1],
                                                    acc[t][1][2 * i + 1], p, rnd[i], shv[i]);
                    *(uint16_t *)(stage + (2 * g + i) * (2 * G) + 2 * jt) = (uint16_t)v;
                }
            }
        }
        chz_wave_fence();
        if (st_ch != CHZ_NONE) {
#pragma unroll
            for (uint32_t s = 0; s < 2 * G / 128; s++) {
                const uint4 v = *(const uint4 *)(stage + st_cl * (2 * G) + 128 * s + 16 * st_piece);
                *(uint4 *)(a.out + (size_t)st_ch * a.out_row + 2 * (size_t)(m0 + grp * G) + 128 * s + 16 * st_piece) = v;
            }
        }
        chz_wave_fence();
    }
}

// chz_kernel for a fractional decimation P / Q: blocks of t_blk outputs (a multiple of chz_frac_group(Q)), the window of
// their t_blk / Q wide steps staged exactly as for the integer decimator by P.
template <int Q>
__global__ __launch_bounds__(512) void chz_frac_kernel(const ChzLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t chz_lds[];
    constexpr uint32_t G = chz_frac_group(Q);
    uint32_t *sp = (uint32_t *)chz_lds;
    uint8_t *stage_all = chz_lds + CHZ_PHASOR * 4;
    uint8_t *win = chz_lds + CHZ_PHASOR * 4 + CHZ_FRAC_STAGE;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const ChzWg w = a.wgs[blockIdx.y];
    const uint32_t m0 = blockIdx.x * a.t_blk;
    const uint32_t nloc = min(a.t_blk, a.n_out - m0);           // a multiple of 32 Q: whole groups
    const uint32_t nq = a.nq;

    for (uint32_t i = tid; i < CHZ_PHASOR / 4; i += blockDim.x) ((uint4 *)sp)[i] = ((const uint4 *)a.phasor)[i];
    chz_stage_window(a, w.source, m0 / Q, nloc / Q, win);
    __syncthreads();
    if (wave >= w.n_tiles) return;

    const uint32_t tile = w.first_tile + wave;
    const ChzTile *T = a.tiles + tile;
    const uint32_t g = lane >> 4;
    uint32_t inc[2], shv[2];
    int32_t rnd[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        inc[i] = T->inc[2 * g + i];
        const uint32_t L = T->shift[2 * g + i];
        shv[i] = 22 - L;
        rnd[i] = 1 << (21 - L);
    }
    const uint32_t st_ch = T->ch[lane >> 3];
    uint8_t *stage = stage_all + wave * (CHZ_TILE_CH * 2 * G);
    const uint4 *amat = a.amat + (size_t)tile * Q * nq * 2 * 64 + lane;
    chz_frac_tile_outputs<Q>(a, win, sp, stage, amat, inc, shv, rnd, st_ch, m0, nloc);
}

hipError_t launch_channelizer_frac(const ChzLaunch &a, uint32_t n_wgs, hipStream_t s)
{
    const dim3 grid((a.n_out + a.t_blk - 1) / a.t_blk, n_wgs);
    const size_t lds = CHZ_PHASOR * 4 + CHZ_FRAC_STAGE + 2 * ((size_t)a.t_blk / a.den * a.m + a.kp) + 16;
    if (a.den == 2) hipLaunchKernelGGL(chz_frac_kernel<2>, grid, dim3(512), lds, s, a);
    else if (a.den == 4) hipLaunchKernelGGL(chz_frac_kernel<4>, grid, dim3(512), lds, s, a);
    else if (a.den == 8) hipLaunchKernelGGL(chz_frac_kernel<8>, grid, dim3(512), lds, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace iqd
