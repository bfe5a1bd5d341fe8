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
// Of the pieces of iqd_chan_dev.h: chz_stage_window<CHZ_S8 / CHZ_S16>, chz_walk<1, NQR, PLANES, ...> with ChzRowSink<1, false> and
// ChzFinish (S8) or ChzFinishS16 below.
//
// The history is raw capture bytes (the last Kp samples, 2 Kp B bytes per source; zero history is zero bytes) and goes
// through the same staging.  LDS is chz_kernel's: the planes share CHZ_WIN_MAX, so an S16 window covers half the outputs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan.h"
#include "iqd_chan_dev.h"

namespace iqd {

// Finish of chz_walk for S16.  acc[s][p]: sample plane s (0 = hi, 1 = lo'), tap plane p (0 = lo, 1 = hi); gs[i]: the
// coefficient sums of the rows (re, im) of the lane's channel i.
struct ChzFinishS16 {
    ChzFinish fin;
    int32_t gs[2][2];
    __device__ __forceinline__ uint32_t operator()(const chz_v4i (&acc)[2][2], int i, uint32_t p) const
    {
        const int32_t vr = chz_fmt_stage_a(acc[0][0][2 * i], acc[0][1][2 * i], acc[1][0][2 * i], acc[1][1][2 * i], gs[i][0]);
        const int32_t vi = chz_fmt_stage_a(acc[0][0][2 * i + 1], acc[0][1][2 * i + 1], acc[1][0][2 * i + 1], acc[1][1][2 * i + 1],
                                           gs[i][1]);
        return chz_epilogue(0, vr, 0, vi, p, fin.rnd[i], fin.shv[i]);   // (256 v + 128) >> 8 = v: sat16 and on
    }
};

template <int PLANES, int NQR>   // NQR > 0: nq <= NQR, the A operands stay in registers; 0: they are read per group
__global__ __launch_bounds__(512) void chz_fmt_kernel(const ChzFmtLaunch f)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t chz_lds[];
    const ChzLaunch &a = f.a;
    uint32_t *sp = (uint32_t *)chz_lds;
    uint8_t *stage_all = chz_lds + CHZ_PHASOR * 4;
    uint8_t *win = chz_lds + CHZ_LDS_FIXED;
    const uint32_t wave = threadIdx.x >> 6, g = (threadIdx.x & 63) >> 4;
    const ChzWg w = a.wgs[blockIdx.y];
    const uint32_t m0 = blockIdx.x * a.t_blk;
    const uint32_t nloc = min(a.t_blk, a.n_out - m0);           // a multiple of 32

    chz_phasor_to_lds(a, sp);
    chz_stage_window<PLANES == 2 ? CHZ_S16 : CHZ_S8>(a, w.source, m0, nloc, win, f.pstride);
    __syncthreads();
    if (wave >= w.n_tiles) return;

    const uint32_t tile = w.first_tile + wave;
    ChzLaneTile<NQR> T;
    T.params(a, tile, 1, true);
    T.load_a(a.nq);
    ChzRowSink<1, false> sink{stage_all + wave * (CHZ_TILE_CH * 2 * CHZ_GROUP), T.st_ch, 0};
    if constexpr (PLANES == 2) {
        const int32_t (&gs)[CHZ_TILE_CH][2] = f.gsum[tile].g;
        const ChzFinishS16 fin{T.fin, {{gs[2 * g][0], gs[2 * g][1]}, {gs[2 * g + 1][0], gs[2 * g + 1][1]}}};
        chz_walk<1, NQR, 2, CHZ_CONSECUTIVE>(a, win, f.pstride, sp, T.A, T.amat, T.inc, m0, nloc, 0, 1, fin, sink);
    } else {
        chz_walk<1, NQR, 1, CHZ_CONSECUTIVE>(a, win, 0, sp, T.A, T.amat, T.inc, m0, nloc, 0, 1, T.fin, sink);
    }
}

hipError_t launch_channelizer_fmt(const ChzFmtLaunch &f, uint32_t n_wgs, hipStream_t st)
{
    const ChzLaunch &a = f.a;
    if (a.rail_bytes != 1 && a.rail_bytes != 2) return hipErrorInvalidValue;
    const uint32_t planes = a.rail_bytes;
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
    return launch_channelizer_history(a, st);                   // (iqd_chan.hip)
}

}  // namespace iqd
