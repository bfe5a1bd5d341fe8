// Wideband channelizer at a fractional decimation P / Q, Q = 2, 4, 8 (include/iqdemod.h: "Fractional decimation"; layout of
// the operands: iqd_chan.h).  A decimator by P / Q is Q interleaved integer decimators by P with different tap sets: the
// outputs m = rho + Q t of residue rho use branch ((rho + 1) P - 1) mod Q at n = P t + floor(((rho + 1) P - 1) / Q).  Grid,
// window staging, MFMA / epilogue / 16-byte stores as chz_kernel (iqd_chan.hip); what differs: the 16 columns of one MFMA
// are 16 outputs of ONE residue (window stride 2 P bytes), its A operand is that residue's tap set, read per group, and a
// store group is 16 max(4, Q) consecutive outputs assembled from the Q residues in the wave's staging row: chz_walk<Q, 0, 1, ...>
// with ChzFinish and ChzRowSink<Q, false> (iqd_chan_dev.h).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan.h"
#include "iqd_chan_dev.h"

namespace iqd {

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
    const uint32_t wave = threadIdx.x >> 6;
    const ChzWg w = a.wgs[blockIdx.y];
    const uint32_t m0 = blockIdx.x * a.t_blk;
    const uint32_t nloc = min(a.t_blk, a.n_out - m0);           // a multiple of 32 Q: whole groups

    chz_phasor_to_lds(a, sp);
    chz_stage_window<CHZ_U8>(a, w.source, m0 / Q, nloc / Q, win);
    __syncthreads();
    if (wave >= w.n_tiles) return;

    // the A operands of the residues are read per group (Q sets of nq chunks do not stay in registers)
    ChzLaneTile<0> T;
    T.params(a, w.first_tile + wave, Q, true);
    ChzRowSink<Q, false> sink{stage_all + wave * (CHZ_TILE_CH * 2 * G), T.st_ch, 0};
    chz_walk<Q, 0, 1, CHZ_PER_RESIDUE>(a, win, 0, sp, T.A, T.amat, T.inc, m0, nloc, 0, 1, T.fin, sink);
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
