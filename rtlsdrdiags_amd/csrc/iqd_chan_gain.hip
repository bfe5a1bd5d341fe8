// Gain-following channels of the wideband channelizer (include/iqdemod.h: iqd_channelizer_follow_gain).
//
// The gain walker.  One workgroup owns up to g.waves tiles of gain-following channels of one source for the whole call and
// walks its blocks in order, g.wpt waves per tile (each takes every g.wpt-th group of 64 outputs of a window and keeps its
// own, identical, shadow copy).  The tiles' A operands are the host-packed ones of the fixed path, loaded once per call.
// Per block
//   1. the lane that owns a channel's shadow state (lane 8 l of the tile's wave for slot l; the state itself waits in LDS,
//      out of the registers the MFMA loop needs) turns its current IF gain g = min(G, 48) into mantissa and exponent
//      (m_j, e); they travel to the lanes that compute the channel by __shfl;
//   2. the block's outputs, window by window (chz_walk<1, NQR, 1, ...> with ChzFinishGain below and ChzRowSink<1, true>,
//      iqd_chan_dev.h): the MFMAs and the epilogue of chz_kernel up to rr / ri, then the dB step
//      y = sat8((floor(r m_j / 2^14) + 2^(19 - e)) >> (20 - e)), the staging row, the 16-byte stores and the squelch's
//      magnitude of the stored bytes;
//   3. the magnitude sums meet in LDS and the owner lanes step the shadow copy of their engine channel's AGC in
//      squelch_track_kernel's order: agc_run on the block's magnitude with the gain in force.
// The shadow state is dropped at the end: iqd_accept_iq_device on the rows re-derives the same decisions for real.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan.h"
#include "iqd_chan_dev.h"
#include "iqd_chains.h"

namespace iqd {

// Finish of chz_walk with the gain in dB: chz_epilogue up to the rotation, then m18[i] = m_j << 18, shv[i] = 20 - e of the
// lane's two channels (the rounding constant 2^(19 - e) is 1 << (shv - 1)).
struct ChzFinishGain {
    int32_t m18[2];
    uint32_t shv[2];
    __device__ __forceinline__ uint32_t operator()(const chz_v4i (&acc)[1][2], int i, uint32_t p) const
    {
        int32_t rr, ri;
        chz_epilogue_rot(acc[0][0][2 * i], acc[0][1][2 * i], acc[0][0][2 * i + 1], acc[0][1][2 * i + 1], p, rr, ri);
        const int32_t rnd = 1 << (shv[i] - 1);
        const int32_t yr = chz_gain_rail(rr, m18[i], rnd, shv[i]);
        const int32_t yi = chz_gain_rail(ri, m18[i], rnd, shv[i]);
        return (uint32_t)((yr + 128) | ((yi + 128) << 8));
    }
};

template <int NQR>   // NQR > 0: nq <= NQR, the A operands stay in registers; 0: they are read per group
__global__ __launch_bounds__(512) void chz_gain_kernel(const ChzLaunch a, const ChzGainLaunch s)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t chz_lds[];
    uint32_t *sp = (uint32_t *)chz_lds;
    uint8_t *stage_all = chz_lds + CHZ_PHASOR * 4;
    uint32_t *magsum = (uint32_t *)(chz_lds + CHZ_LDS_FIXED);   // [2][CHZ_WAVES * 8], by block parity
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    ChzGainShadow *shadow = (ChzGainShadow *)(chz_lds + CHZ_LDS_FIXED + CHZ_SCAN_MAGSUM) + (tid >> 3);   // [CHZ_WAVES * 8]
    uint8_t *win = chz_lds + CHZ_LDS_FIXED + CHZ_SCAN_MAGSUM + CHZ_GAIN_SHADOW;
    const uint32_t tl = (tid >> 6) / s.wpt, part = (tid >> 6) % s.wpt;   // tile of the workgroup, share of its outputs
    const ChzWg w = a.wgs[blockIdx.x];

    chz_phasor_to_lds(a, sp);

    const bool active = tl < w.n_tiles;
    ChzLaneTile<NQR> T;
    T.params(a, w.first_tile + (active ? tl : 0), 1, active);
    const uint32_t g = lane >> 4, st_ch = T.st_ch;
    uint8_t *stage = stage_all + (tid >> 6) * (CHZ_TILE_CH * 2 * CHZ_GROUP);

    // the shadow state of each channel: its owner lane's entry in LDS (st.rx_gain is the gain in force)
    const bool owner = (lane & 7) == 0 && st_ch != CHZ_NONE;
    if (owner) {
        shadow->cfg = s.agc_cfg[s.first_ch + st_ch];
        shadow->st = s.agc[s.first_ch + st_ch];
    }
    const Consts &cst = *s.consts;

    T.load_a(a.nq);
    for (uint32_t b = 0; b < s.n_blocks; b++) {
        // 1. this block's gain as (m_j, e); a lane that owns nothing sends 0: its outputs are never stored
        const uint32_t me = owner ? chz_gain_split(min(shadow->st.rx_gain, (uint32_t)IQD_GAIN_FOLLOW_MAX)) : 0u;
        ChzFinishGain fin;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint32_t v = (uint32_t)__shfl((int)me, (int)(8 * (2 * g + i)));
            fin.m18[i] = (int32_t)((v >> 4) << 18);
            fin.shv[i] = 20 - (v & 15u);
        }
        chz_block_open(magsum, b);
        __syncthreads();   // (the phasor table; and the previous block's last window has been read)
        // 2. the block's outputs, window by window
        ChzRowSink<1, true> sink{stage, st_ch, 0};
        const uint32_t mb = b * s.block_out, mend = mb + s.block_out;
        for (uint32_t m0 = mb; m0 < mend; m0 += s.t_blk) {
            const uint32_t nloc = min(s.t_blk, mend - m0);
            if (m0 != mb) __syncthreads();
            chz_stage_window<CHZ_U8>(a, w.source, m0, nloc, win);
            __syncthreads();
            if (active) chz_walk<1, NQR, 1, CHZ_CONSECUTIVE>(a, win, 0, sp, T.A, T.amat, T.inc, m0, nloc, part, s.wpt, fin, sink);
        }
        // 3. the squelch's magnitude per channel, then the shadow step
        const uint32_t *ms = chz_block_close(magsum, b, tl, sink.mag, owner);
        if (owner && shadow->cfg.enabled) {
            const AgcConfig cfg = shadow->cfg;
            AgcState st = shadow->st;
            st.rx_gain = agc_run(cst, cfg, st, *ms / s.block_out, st.rx_gain);
            shadow->st = st;
        }
    }
}

hipError_t launch_channelizer_gain(const ChzLaunch &a, uint32_t n_wgs, const ChzGainLaunch &g, hipStream_t st)
{
    if (!n_wgs) return hipSuccess;
    const size_t lds = CHZ_LDS_FIXED + CHZ_SCAN_MAGSUM + CHZ_GAIN_SHADOW + 2 * ((size_t)g.t_blk * a.m + a.kp) + 16;
    const dim3 block(64 * g.waves * g.wpt);
    if (a.nq <= CHZ_NQ_REG) hipLaunchKernelGGL(chz_gain_kernel<CHZ_NQ_REG>, dim3(n_wgs), block, lds, st, a, g);
    else hipLaunchKernelGGL(chz_gain_kernel<0>, dim3(n_wgs), block, lds, st, a, g);
    return hipGetLastError();
}

}  // namespace iqd
