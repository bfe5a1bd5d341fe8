// Gain-following channels of the wideband channelizer (include/iqdemod.h: iqd_channelizer_follow_gain).
//
// The gain walker.  One workgroup owns up to g.waves tiles of gain-following channels of one source for the whole call and
// walks its blocks in order, g.wpt waves per tile (each takes every g.wpt-th group of 64 outputs of a window and keeps its
// own, identical, shadow copy).  The tiles' A operands are the host-packed ones of the fixed path, loaded once per call.
// Per block
//   1. the lane that owns a channel's shadow state (lane 8 l of the tile's wave for slot l; the state itself waits in LDS,
//      out of the registers the MFMA loop needs) turns its current IF gain g = min(G, 48) into mantissa and exponent
//      (m_j, e); they travel to the lanes that compute the channel by __shfl;
//   2. the block's outputs, window by window: the MFMAs and the epilogue of chz_kernel up to rr / ri, then the dB step
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

// One wave: its tile's outputs [m0, m0 + nloc) (nloc a multiple of 32), every gstride-th group of 64 from grp0, from the
// staged window.  chz_tile_outputs (iqd_chan.hip) with the gain in dB: m18[i] = m_j << 18, shv[i] = 20 - e of the lane's
// two channels (the rounding constant 2^(19 - e) is 1 << (shv - 1)).
template <int NQR>
__device__ __forceinline__ void chz_gain_outputs(const ChzLaunch &a, const uint8_t *win, const uint32_t *sp, uint8_t *stage,
                                                 const chz_v4i (&A)[NQR > 0 ? NQR : 1][2], const uint4 *amat,
                                                 const uint32_t (&inc)[2], const int32_t (&m18)[2], const uint32_t (&shv)[2],
                                                 uint32_t st_ch, uint32_t m0, uint32_t nloc, uint32_t &mag, uint32_t grp0,
                                                 uint32_t gstride)
{
    const uint32_t lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const uint32_t st_cl = lane >> 3, st_piece = lane & 7;
    const uint32_t M = a.m, nq = a.nq;
    const chz_v4i zero = {0, 0, 0, 0};
    for (uint32_t grp = grp0; grp * CHZ_GROUP < nloc; grp += gstride) {
        const uint32_t ntl = min(4u, (nloc - grp * CHZ_GROUP) / 16);   // 2 or 4
        for (uint32_t tp = 0; tp < ntl; tp += 2) {
            chz_v4i acc[2][2] = {{zero, zero}, {zero, zero}};
            const uint32_t obase = 2 * M * (grp * CHZ_GROUP + 16 * tp + col + 1) + 16 * g;
            if (NQR > 0) {
#pragma unroll
                for (int q = 0; q < NQR; q++)
                    if (q < (int)nq) {
#pragma unroll
                        for (int t = 0; t < 2; t++) {
                            const chz_v4i b = chz_b_operand(win, obase + 2 * M * 16 * t + 64 * q);
                            acc[t][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[q][0], b, acc[t][0], 0, 0, 0);
                            acc[t][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[q][1], b, acc[t][1], 0, 0, 0);
                        }
                    }
            } else {
                for (uint32_t q = 0; q < nq; q++) {
                    const chz_v4i alo = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 0) * 64]);
                    const chz_v4i ahi = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 1) * 64]);
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const chz_v4i b = chz_b_operand(win, obase + 2 * M * 16 * t + 64 * q);
                        acc[t][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(alo, b, acc[t][0], 0, 0, 0);
                        acc[t][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ahi, b, acc[t][1], 0, 0, 0);
                    }
                }
            }
            // epilogue: lane (col, g) holds rows 4 g .. 4 g + 3 = channels 2 g, 2 g + 1 (re, im) of output col of each tile
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const uint32_t jt = 16 * (tp + t) + col;                       // output within the group
                const uint32_t n32 = a.nbase + (m0 + grp * CHZ_GROUP + jt) * M + M - 1;   // mod 2^32
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const uint32_t p = sp[(n32 * inc[i]) >> 20];
                    int32_t rr, ri;
                    chz_epilogue_rot(acc[t][0][2 * i], acc[t][1][2 * i], acc[t][0][2 * i + 1], acc[t][1][2 * i + 1], p, rr, ri);
                    const int32_t rnd = 1 << (shv[i] - 1);
                    const int32_t yr = chz_gain_rail(rr, m18[i], rnd, shv[i]);
                    const int32_t yi = chz_gain_rail(ri, m18[i], rnd, shv[i]);
                    *(uint16_t *)(stage + (2 * g + i) * (2 * CHZ_GROUP) + 2 * jt) = (uint16_t)((yr + 128) | ((yi + 128) << 8));
                }
            }
        }
        chz_wave_fence();
        if (st_ch != CHZ_NONE && st_piece * 8 < ntl * 16) {
            const uint4 v = *(const uint4 *)(stage + st_cl * (2 * CHZ_GROUP) + 16 * st_piece);
            *(uint4 *)(a.out + (size_t)st_ch * a.out_row + 2 * (size_t)(m0 + grp * CHZ_GROUP) + 16 * st_piece) = v;
            mag += magnitude2(v.x ^ 0x80808080u) + magnitude2(v.y ^ 0x80808080u) + magnitude2(v.z ^ 0x80808080u) +
                   magnitude2(v.w ^ 0x80808080u);
        }
        chz_wave_fence();
    }
}

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
    const uint32_t nq = a.nq;

    for (uint32_t i = tid; i < CHZ_PHASOR / 4; i += blockDim.x) ((uint4 *)sp)[i] = ((const uint4 *)a.phasor)[i];

    const bool active = tl < w.n_tiles;
    const uint32_t tile = w.first_tile + (active ? tl : 0);
    const ChzTile *T = a.tiles + tile;
    const uint32_t g = lane >> 4;
    const uint32_t inc[2] = {T->inc[2 * g], T->inc[2 * g + 1]};
    const uint32_t st_ch = active ? T->ch[lane >> 3] : CHZ_NONE;
    uint8_t *stage = stage_all + (tid >> 6) * (CHZ_TILE_CH * 2 * CHZ_GROUP);
    const uint4 *amat = a.amat + (size_t)tile * nq * 2 * 64 + lane;

    // the shadow state of each channel: its owner lane's entry in LDS (st.rx_gain is the gain in force)
    const bool owner = (lane & 7) == 0 && st_ch != CHZ_NONE;
    if (owner) {
        shadow->cfg = s.agc_cfg[s.first_ch + st_ch];
        shadow->st = s.agc[s.first_ch + st_ch];
    }
    const Consts &cst = *s.consts;

    chz_v4i A[NQR > 0 ? NQR : 1][2];
    if (NQR > 0) {
#pragma unroll
        for (int q = 0; q < NQR; q++)
            if (q < (int)nq) {
                A[q][0] = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 0) * 64]);
                A[q][1] = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 1) * 64]);
            }
    }
    for (uint32_t b = 0; b < s.n_blocks; b++) {
        // 1. this block's gain as (m_j, e); a lane that owns nothing sends 0: its outputs are never stored
        const uint32_t me = owner ? chz_gain_split(min(shadow->st.rx_gain, (uint32_t)IQD_GAIN_FOLLOW_MAX)) : 0u;
        int32_t m18[2];
        uint32_t shv[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint32_t v = (uint32_t)__shfl((int)me, (int)(8 * (2 * g + i)));
            m18[i] = (int32_t)((v >> 4) << 18);
            shv[i] = 20 - (v & 15u);
        }
        if (tid < CHZ_WAVES * 8) magsum[(b & 1) * CHZ_WAVES * 8 + tid] = 0;
        __syncthreads();   // (the phasor table; and the previous block's last window has been read)
        // 2. the block's outputs, window by window
        uint32_t mag = 0;
        const uint32_t mb = b * s.block_out, mend = mb + s.block_out;
        for (uint32_t m0 = mb; m0 < mend; m0 += s.t_blk) {
            const uint32_t nloc = min(s.t_blk, mend - m0);
            if (m0 != mb) __syncthreads();
            chz_stage_window(a, w.source, m0, nloc, win);
            __syncthreads();
            if (active) chz_gain_outputs<NQR>(a, win, sp, stage, A, amat, inc, m18, shv, st_ch, m0, nloc, mag, part, s.wpt);
        }
        // 3. the squelch's magnitude per channel (its 8 storing lanes), then the shadow step
        mag += (uint32_t)__shfl_xor((int)mag, 1);
        mag += (uint32_t)__shfl_xor((int)mag, 2);
        mag += (uint32_t)__shfl_xor((int)mag, 4);
        uint32_t *ms = magsum + (b & 1) * CHZ_WAVES * 8 + tl * 8 + (lane >> 3);
        if (owner) atomicAdd(ms, mag);
        __syncthreads();
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
