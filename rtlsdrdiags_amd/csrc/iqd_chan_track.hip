// Track-following channels of the wideband channelizer (include/iqdemod.h: iqd_channelizer_follow_tracks).
//
// A following channel's row is cut block by block at the increments a slot table holds (iqd_track_run_device's output, or
// any table of that layout).  The table is complete before the kernel starts, so nothing is walked in order: every
// (table block, window of the block, workgroup row of up to 8 tiles of one source) is a workgroup of its own, chz_kernel's
// geometry with the block as one more grid factor.  A workgroup
//   1. stages the phasor table, the prototype and its window in LDS;
//   2. per tile (wave): the lane that stores a channel's row (lane 8 l for slot l) reads `state` and `phase_inc` of the
//      table entry its channel follows for this block - or, for block 0 at lag 1, the channel's carry - and the decision
//      (live, d) travels to the lanes that need it by __shfl;
//   3. builds the tile's A operands for those increments - exactly chz_pack_slot's bytes; a slot that is not live gets zero
//      taps, which is 0x80 in every output byte - in registers for nq <= CHZ_NQ_REG; for larger K chz_track_build_kernel has
//      written them per (table block, tile) into a scratch buffer before, and the kernel reads its slice;
//   4. one chz_walk<1, NQR, 1, CHZ_CONSECUTIVE> with ChzFinish and ChzRowSink<1, false> (iqd_chan_dev.h).
// The workgroups of the call's last table block (window 0) also write the next call's carry - the decision of table entry
// n_blocks - 1 whatever the lag - into the other half of a double buffer, which the host swaps per call: no workgroup of
// this call reads what another one writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan.h"
#include "iqd_chan_dev.h"
#include "iqd_chains.h"

namespace iqd {

// This lane's part of one K-chunk q of a tile's A operands for the increment d of slot (lane & 15) >> 1, row (lane & 15) & 1
// (Ar / Ai), both tap planes: K-index kappa = 64 q + 16 g + j is sample kp - 1 - kappa / 2, rail kappa & 1 (iqd_chan.h).
// The scan walker's `build` (iqd_chan.hip), here as a function of its own: proto [kp] and the phasor table sp in LDS
// (chz_track_kernel) or in device memory (chz_track_build_kernel).
__device__ __forceinline__ void chz_track_build(const int16_t *proto, const uint32_t *sp, uint32_t kp, uint32_t q, bool live,
                                                uint32_t d, uint4 &vlo, uint4 &vhi)
{
    const uint32_t lane = threadIdx.x & 63, g = lane >> 4, a_row = lane & 1;
    uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
    if (live) {
#pragma unroll
        for (uint32_t j = 0; j < 8; j++) {
            const uint32_t kk = kp - 1 - 32 * q - 8 * g - j;
            const int32_t h = proto[kk];
            const uint32_t p = sp[(kk * d) >> 20];
            const int32_t gr = (h * (int32_t)(int16_t)(p & 0xffffu) + (1 << 14)) >> 15;
            const int32_t gi = (h * (int32_t)(int16_t)(p >> 16) + (1 << 14)) >> 15;
            const int32_t v0 = a_row == 0 ? gr : gi, v1 = a_row == 0 ? -gi : gr;
            // the two signed-byte planes: v = 256 hi + lo, lo = (int8) v
            const uint32_t l2 = (uint32_t)(v0 & 0xff) | (uint32_t)(v1 & 0xff) << 8;
            const uint32_t h2 = (uint32_t)(((v0 - (int8_t)v0) >> 8) & 0xff) | (uint32_t)(((v1 - (int8_t)v1) >> 8) & 0xff) << 8;
            lo[j >> 1] |= l2 << (16 * (j & 1));
            hi[j >> 1] |= h2 << (16 * (j & 1));
        }
    }
    vlo = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    vhi = make_uint4(hi[0], hi[1], hi[2], hi[3]);
}

// The decision for slot l = lane >> 3 of `tile` at table block b, in every lane of the wave (the eight lanes of a slot
// hold the same): live (0 / 1) and the increment d.  ChzTile::inc of a track tile holds the table slot the channel follows
// and CHZ_TRACK_FRESH (the channel has just started to follow: its carry is not live).  entry: the table block to read,
// or -1 for the carry.
__device__ __forceinline__ void chz_track_decide(const ChzLaunch &a, const ChzTrackLaunch &t, uint32_t tile, uint32_t source,
                                                 int64_t entry, uint32_t &live, uint32_t &d)
{
    const uint32_t l = (threadIdx.x & 63) >> 3;
    const ChzTile *T = a.tiles + tile;
    const uint32_t ch = T->ch[l], slot = T->inc[l];
    live = 0;
    d = 0;
    if (ch == CHZ_NONE) return;
    if (entry < 0) {
        const uint2 c = t.carry[ch];
        if (!(slot & CHZ_TRACK_FRESH)) {
            live = c.x;
            d = c.y;
        }
    } else {
        const uint32_t *e = (const uint32_t *)(t.slots + ((size_t)source * t.n_blocks + (size_t)entry) * t.n_slots +
                                               (slot & ~CHZ_TRACK_FRESH));
        const uint32_t state = e[1] & 0xffu;            // iqd_track_slot: track_id | state, flags, hits, width_class | ...
        live = state >= t.min_state ? 1u : 0u;
        d = live ? e[4] : 0u;                           // ... | misses, max_width | centre_q8 | phase_inc
    }
}

template <int NQR>   // NQR > 0: nq <= NQR, the A operands are built in registers; 0: read per group from t.amat's slice
__global__ __launch_bounds__(512) void chz_track_kernel(const ChzLaunch a, const ChzTrackLaunch t)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t chz_lds[];
    uint32_t *sp = (uint32_t *)chz_lds;
    uint8_t *stage_all = chz_lds + CHZ_PHASOR * 4;
    int16_t *proto = (int16_t *)(chz_lds + CHZ_LDS_FIXED);
    uint8_t *win = chz_lds + CHZ_LDS_FIXED + 2 * CHZ_PROTO_MAX;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const ChzWg w = a.wgs[blockIdx.y];
    const uint32_t b = t.b0 + blockIdx.x / t.wins, wi = blockIdx.x % t.wins;   // table block, window of the block
    const uint32_t m0 = b * t.block_out + wi * a.t_blk;
    const uint32_t nloc = min(a.t_blk, t.block_out - wi * a.t_blk);            // a multiple of 32

    chz_phasor_to_lds(a, sp);
    if (NQR > 0)
        for (uint32_t i = threadIdx.x; i < a.kp / 8; i += blockDim.x) ((uint4 *)proto)[i] = ((const uint4 *)t.proto)[i];
    chz_stage_window<CHZ_U8>(a, w.source, m0, nloc, win);
    __syncthreads();
    if (wave >= w.n_tiles) return;

    const uint32_t tile = w.first_tile + wave;
    ChzLaneTile<NQR> T;                                          // (its increments and A operands are set here)
    T.params(a, tile, 1, true);
    uint32_t live, d;
    chz_track_decide(a, t, tile, w.source, (int64_t)b - (int64_t)t.lag, live, d);
    if (b + 1 == t.n_blocks && wi == 0) {                        // the next call's carry: the last table entry's decision
        uint32_t cl = live, cd = d;
        if (t.lag) chz_track_decide(a, t, tile, w.source, (int64_t)b, cl, cd);
        if ((lane & 7) == 0 && T.st_ch != CHZ_NONE) t.carry_next[T.st_ch] = make_uint2(cl, cd);
    }
    const uint32_t g = lane >> 4, a_slot = (lane & 15) >> 1;
#pragma unroll
    for (int i = 0; i < 2; i++) T.inc[i] = (uint32_t)__shfl((int)d, (int)(8 * (2 * g + i)));
    if (NQR > 0) {
        const uint32_t d_a = (uint32_t)__shfl((int)d, (int)(8 * a_slot));
        const bool live_a = __shfl((int)live, (int)(8 * a_slot)) != 0;
#pragma unroll
        for (int q = 0; q < NQR; q++)
            if (q < (int)a.nq) {
                uint4 vlo, vhi;
                chz_track_build(proto, sp, a.kp, (uint32_t)q, live_a, d_a, vlo, vhi);
                T.A[q][0] = __builtin_bit_cast(chz_v4i, vlo);
                T.A[q][1] = __builtin_bit_cast(chz_v4i, vhi);
            }
    } else {
        T.amat = t.amat + ((size_t)(b - t.b0) * t.n_tiles + (tile - t.first_tile)) * a.nq * 2 * 64 + lane;
    }
    ChzRowSink<1, false> sink{stage_all + wave * (CHZ_TILE_CH * 2 * CHZ_GROUP), T.st_ch, 0};
    chz_walk<1, NQR, 1, CHZ_CONSECUTIVE>(a, win, 0, sp, T.A, T.amat, T.inc, m0, nloc, 0, 1, T.fin, sink);
}

// Large K (nq > CHZ_NQ_REG): workgroup (table block of the run, workgroup row), one wave per tile, writes the tiles' A
// operands for that block into t.amat, [run blocks][n_tiles][nq][2 planes] 64 lanes apart.  The prototype and the phasor
// table are read from device memory: this path has to be right, not fast.
__global__ __launch_bounds__(512) void chz_track_build_kernel(const ChzLaunch a, const ChzTrackLaunch t)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63, a_slot = (lane & 15) >> 1;
    const ChzWg w = a.wgs[blockIdx.y];
    if (wave >= w.n_tiles) return;
    const uint32_t rb = blockIdx.x, tile = w.first_tile + wave, b = t.b0 + rb;
    uint32_t live, d;
    chz_track_decide(a, t, tile, w.source, (int64_t)b - (int64_t)t.lag, live, d);
    const uint32_t d_a = (uint32_t)__shfl((int)d, (int)(8 * a_slot));
    const bool live_a = __shfl((int)live, (int)(8 * a_slot)) != 0;
    uint4 *amat = t.amat + ((size_t)rb * t.n_tiles + (tile - t.first_tile)) * a.nq * 2 * 64 + lane;
    for (uint32_t q = 0; q < a.nq; q++) {
        uint4 vlo, vhi;
        chz_track_build(t.proto, a.phasor, a.kp, q, live_a, d_a, vlo, vhi);
        amat[(q * 2 + 0) * 64] = vlo;
        amat[(q * 2 + 1) * 64] = vhi;
    }
}

hipError_t launch_channelizer_track(const ChzLaunch &a, uint32_t n_wgs, const ChzTrackLaunch &t, uint32_t run_blocks, hipStream_t st)
{
    if (!n_wgs) return hipSuccess;
    const size_t lds = CHZ_LDS_FIXED + 2 * CHZ_PROTO_MAX + 2 * ((size_t)a.t_blk * a.m + a.kp) + 16;
    if (a.nq <= CHZ_NQ_REG) {   // one launch whatever the number of blocks
        hipLaunchKernelGGL(chz_track_kernel<CHZ_NQ_REG>, dim3(t.n_blocks * t.wins, n_wgs), dim3(512), lds, st, a, t);
        return hipGetLastError();
    }
    for (uint32_t b0 = 0; b0 < t.n_blocks; b0 += run_blocks) {   // runs of blocks: the scratch holds run_blocks x n_tiles slices
        ChzTrackLaunch r = t;
        r.b0 = b0;
        const uint32_t nb = min(run_blocks, t.n_blocks - b0);
        hipLaunchKernelGGL(chz_track_build_kernel, dim3(nb, n_wgs), dim3(512), 0, st, a, r);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(chz_track_kernel<0>, dim3(nb * t.wins, n_wgs), dim3(512), lds, st, a, r);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace iqd
