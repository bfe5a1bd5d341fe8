// Band survey of the wideband channelizer (include/iqdemod.h: iqd_channelizer_survey*; layout of the operands: iqd_chan.h).
//
// A survey point is a virtual channel measured on every source: the kernel runs chz_kernel's / chz_frac_kernel's window
// staging, MFMAs and epilogue, and instead of storing the byte pair it takes SignalDetector's magnitude of it where the
// epilogue leaves it - in the lane.  No staging row, no rows in HBM.
//
// Grid: one workgroup per (source, window of t_blk outputs, row of up to 8 point tiles); the point tiles (8 points, one
// wave) are shared by all sources.  One body for every rate: an MFMA tile is 16 outputs of one residue rho of a store
// group (integer decimation: Q = 1, rho = 0, 16 consecutive outputs): chz_walk<Q, NQR, 1, CHZ_PER_RESIDUE> with ChzFinish
// (iqd_chan_dev.h) and the sink below.  The A operands stay in registers at Q = 1 up to CHZ_NQ_REG chunks, else they are
// read per pair of tiles (L2).
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

// Sink of chz_walk: the magnitude of each byte pair, summed in the lane per point; flushed when a pair's block changes
struct ChzSurveySink {
    static constexpr bool UNROLL = false;
    uint32_t *sums;                                             // [n_points] of the source's block being summed
    uint32_t n_points, block_out;
    uint32_t pt[2];                                             // column 0, the lane that adds: its points; else CHZ_NONE
    uint32_t blk_end;                                           // that block's end (outputs; n_out < 2^31)
    uint32_t mag[2];
    __device__ __forceinline__ void flush()
    {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            uint32_t v = mag[i];
            v += (uint32_t)__shfl_xor((int)v, 1);
            v += (uint32_t)__shfl_xor((int)v, 2);
            v += (uint32_t)__shfl_xor((int)v, 4);
            v += (uint32_t)__shfl_xor((int)v, 8);
            if (pt[i] != CHZ_NONE) atomicAdd(sums + pt[i], v);
            mag[i] = 0;
        }
    }
    // the block of this pair's outputs: they begin at mpos and lie in one block
    __device__ __forceinline__ void begin(uint32_t mpos)
    {
        if (mpos >= blk_end) {                                   // (a pair advances by no more than a block)
            flush();
            sums += n_points;
            blk_end += block_out;
        }
    }
    // lane (col, g) holds points 2 g, 2 g + 1 of one output of each tile; its magnitude, not its bytes
    // (the upper pair: signed 0, 0 - magnitude 0)
    __device__ __forceinline__ void put(int i, uint32_t, uint32_t v) { mag[i] += magnitude2(v ^ 0x8080u); }
    __device__ __forceinline__ void end(const ChzLaunch &, uint32_t, uint32_t) {}
};

template <int Q, int NQR>   // NQR > 0 (Q = 1 only): nq <= NQR, the A operands stay in registers
__global__ __launch_bounds__(512) void chz_survey_kernel(const ChzLaunch a, const ChzSurveyLaunch s)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t chz_lds[];
    uint32_t *sp = (uint32_t *)chz_lds;
    uint8_t *win = chz_lds + CHZ_PHASOR * 4;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t x = blockIdx.x;
    const uint32_t row = x % s.rows;
    x /= s.rows;
    const uint32_t m0 = (x % s.n_win) * a.t_blk, source = x / s.n_win;
    const uint32_t nloc = min(a.t_blk, a.n_out - m0);           // Q = 1: a multiple of 32; else whole groups

    chz_phasor_to_lds(a, sp);
    chz_stage_window<CHZ_U8>(a, source, m0 / Q, nloc / Q, win);
    __syncthreads();
    const uint32_t tile = row * CHZ_WAVES + wave;
    if (tile >= s.n_tiles) return;

    ChzLaneTile<NQR> T;
    T.params(a, tile, Q, true);
    T.load_a(a.nq);
    const uint32_t blk = m0 / s.block_out;
    const bool adds = (threadIdx.x & 15) == 0;
    ChzSurveySink sink{s.sums + ((size_t)source * s.n_blocks + blk) * s.n_points, s.n_points, s.block_out,
                       {adds ? T.ch[0] : CHZ_NONE, adds ? T.ch[1] : CHZ_NONE}, (blk + 1) * s.block_out, {0, 0}};
    chz_walk<Q, NQR, 1, CHZ_PER_RESIDUE>(a, win, 0, sp, T.A, T.amat, T.inc, m0, nloc, 0, 1, T.fin, sink);
    sink.flush();
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
