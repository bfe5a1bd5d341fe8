// Band survey of the wideband channelizer (include/iqdemod.h: iqd_channelizer_survey*; layout of the operands: iqd_chan.h).
//
// A survey point is a virtual channel measured on every source: the kernel runs chz_kernel's / chz_frac_kernel's window
// staging, MFMAs and epilogue, and instead of storing the byte pair it takes SignalDetector's magnitude of it where the
// epilogue leaves it - in the lane.  No staging row, no rows in HBM.
//
// Grid: one workgroup per (source, window of t_blk outputs, row of up to 8 point tiles); the point tiles (8 points, one
// wave) are shared by all sources.  One body for every rate: an MFMA tile is 16 outputs of one residue rho of a store
// group (integer decimation: Q = 1, rho = 0, 16 consecutive outputs), exactly chz_frac_tile_outputs' schedule, which at
// Q = 1 is chz_tile_outputs'.  The A operands stay in registers at Q = 1 up to CHZ_NQ_REG chunks, else they are read
// per pair of tiles (L2).
//
// A lane sums the magnitudes of its two points over the outputs it meets; a pair of tiles never crosses a block boundary
// (Q = 1: 32 consecutive outputs and blocks are multiples of 32 outputs; Q > 1: blocks are whole store groups), so the
// wave flushes when the pair's block changes: 16 columns by shuffles, one vector atomicAdd per (window, block, point)
// into the result, which the call zeroed on the stream.  Integer sums: the result does not depend on the order.  A
// second, tiny kernel divides by the block's outputs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan.h"
#include "iqd_chan_dev.h"
#include "iqd_chains.h"

namespace iqd {

template <int Q, int NQR>   // NQR > 0 (Q = 1 only): nq <= NQR, the A operands stay in registers
__global__ __launch_bounds__(512) void chz_survey_kernel(const ChzLaunch a, const ChzSurveyLaunch s)
{
    static_assert(NQR == 0 || Q == 1, "register-resident A operands are for the integer decimator");
    extern __shared__ __attribute__((aligned(16))) uint8_t chz_lds[];
    constexpr uint32_t G = Q == 1 ? CHZ_GROUP : chz_frac_group(Q), NT = G / 16, TG = G / Q;
    uint32_t *sp = (uint32_t *)chz_lds;
    uint8_t *win = chz_lds + CHZ_PHASOR * 4;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, g = lane >> 4;
    uint32_t x = blockIdx.x;
    const uint32_t row = x % s.rows;
    x /= s.rows;
    const uint32_t m0 = (x % s.n_win) * a.t_blk, source = x / s.n_win;
    const uint32_t nloc = min(a.t_blk, a.n_out - m0);           // Q = 1: a multiple of 32; else whole groups
    const uint32_t P = a.m, nq = a.nq, t0 = m0 / Q;

    for (uint32_t i = tid; i < CHZ_PHASOR / 4; i += blockDim.x) ((uint4 *)sp)[i] = ((const uint4 *)a.phasor)[i];
    chz_stage_window(a, source, t0, nloc / Q, win);
    __syncthreads();
    const uint32_t tile = row * CHZ_WAVES + wave;
    if (tile >= s.n_tiles) return;

    const ChzTile *T = a.tiles + tile;
    uint32_t inc[2], shv[2], pt[2], mag[2] = {0, 0};
    int32_t rnd[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        inc[i] = T->inc[2 * g + i];
        const uint32_t L = T->shift[2 * g + i];
        shv[i] = 22 - L;
        rnd[i] = 1 << (21 - L);
        pt[i] = T->ch[2 * g + i];                               // the point, CHZ_NONE = padding
    }
    const uint4 *amat = a.amat + (size_t)tile * Q * nq * 2 * 64 + lane;
    chz_v4i A[NQR > 0 ? NQR : 1][2];
    if (NQR > 0) {
#pragma unroll
        for (int q = 0; q < NQR; q++)
            if (q < (int)nq) {
                A[q][0] = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 0) * 64]);
                A[q][1] = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 1) * 64]);
            }
    }

    uint32_t *sums = s.sums + (size_t)source * s.n_blocks * s.n_points;
    uint32_t blk = m0 / s.block_out, blk_end = (blk + 1) * s.block_out;   // (outputs; n_out < 2^31)
    auto flush = [&]() {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            uint32_t v = mag[i];
            v += (uint32_t)__shfl_xor((int)v, 1);
            v += (uint32_t)__shfl_xor((int)v, 2);
            v += (uint32_t)__shfl_xor((int)v, 4);
            v += (uint32_t)__shfl_xor((int)v, 8);
            if (col == 0 && pt[i] != CHZ_NONE) atomicAdd(sums + (size_t)blk * s.n_points + pt[i], v);
            mag[i] = 0;
        }
    };

    const chz_v4i zero = {0, 0, 0, 0};
    for (uint32_t grp = 0; grp * G < nloc; grp++) {
        const uint32_t ntl = Q == 1 ? min(NT, (nloc - grp * G) / 16) : NT;   // Q = 1: 2 or 4
        for (uint32_t tp = 0; tp < ntl; tp += 2) {
            // the block of this pair's outputs: they begin at mpos and lie in one block
            const uint32_t mpos = m0 + grp * G + (Q == 1 ? 16 * tp : 0);
            if (mpos >= blk_end) {                               // (a pair advances by no more than a block)
                flush();
                blk++;
                blk_end += s.block_out;
            }
            chz_v4i acc[2][2] = {{zero, zero}, {zero, zero}};
            uint32_t e[2], tt[2], ob[2];
            const uint4 *am[2];
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const uint32_t rho = (tp + t) % Q;
                e[t] = ((rho + 1) * P - 1) / Q;
                tt[t] = grp * TG + 16 * ((tp + t) / Q) + col;    // wide step within the window
                ob[t] = 2 * (P * tt[t] + e[t] + 1) + 16 * g;
                am[t] = amat + (size_t)rho * nq * 2 * 64;
            }
            if (NQR > 0) {
#pragma unroll
                for (int q = 0; q < NQR; q++)
                    if (q < (int)nq) {
#pragma unroll
                        for (int t = 0; t < 2; t++) {
                            const chz_v4i b = chz_b_operand(win, ob[t] + 64 * q);
                            acc[t][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[q][0], b, acc[t][0], 0, 0, 0);
                            acc[t][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[q][1], b, acc[t][1], 0, 0, 0);
                        }
                    }
            } else {
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
            }
            // epilogue: lane (col, g) holds points 2 g, 2 g + 1 of one output of each tile; its magnitude, not its bytes
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const uint32_t n32 = a.nbase + (t0 + tt[t]) * P + e[t];      // mod 2^32
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const uint32_t p = sp[(n32 * inc[i]) >> 20];
                    const uint32_t v = chz_epilogue(acc[t][0][2 * i], acc[t][1][2 * i], acc[t][0][2 * i + 1],
                                                    acc[t][1][2 * i + 1], p, rnd[i], shv[i]);
                    mag[i] += magnitude2(v ^ 0x8080u);           // (the upper pair: signed 0, 0 - magnitude 0)
                }
            }
        }
    }
    flush();
}

// sums -> magnitudes: floor(sum / outputs of a block)
__global__ void chz_survey_close_kernel(uint32_t *sums, uint32_t n, uint32_t block_out)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) sums[t] /= block_out;
}

hipError_t launch_channelizer_survey(const ChzLaunch &a, const ChzSurveyLaunch &s, hipStream_t st)
{
    const uint64_t n_wgs = (uint64_t)a.n_sources * s.n_win * s.rows;
    const uint64_t n_res = (uint64_t)a.n_sources * s.n_blocks * s.n_points;
    if (n_wgs == 0 || n_wgs > 0x7fffffffull || n_res > 0xffffffffull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)n_wgs);
    const size_t lds = CHZ_PHASOR * 4 + 2 * ((size_t)a.t_blk / a.den * a.m + a.kp) + 16;
    if (a.den == 1 && a.nq <= CHZ_NQ_REG) hipLaunchKernelGGL((chz_survey_kernel<1, CHZ_NQ_REG>), grid, dim3(512), lds, st, a, s);
    else if (a.den == 1) hipLaunchKernelGGL((chz_survey_kernel<1, 0>), grid, dim3(512), lds, st, a, s);
    else if (a.den == 2) hipLaunchKernelGGL((chz_survey_kernel<2, 0>), grid, dim3(512), lds, st, a, s);
    else if (a.den == 4) hipLaunchKernelGGL((chz_survey_kernel<4, 0>), grid, dim3(512), lds, st, a, s);
    else if (a.den == 8) hipLaunchKernelGGL((chz_survey_kernel<8, 0>), grid, dim3(512), lds, st, a, s);
    else return hipErrorInvalidValue;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(chz_survey_close_kernel, dim3((uint32_t)((n_res + 255) / 256)), dim3(256), 0, st, s.sums, (uint32_t)n_res,
                       s.block_out);
    return hipGetLastError();
}

}  // namespace iqd
