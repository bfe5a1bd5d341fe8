// Wideband channelizer kernel (include/iqdemod.h: iqd_channelizer_*; layout of the operands: iqd_chan.h).
//
// Grid: x = blocks of t_blk outputs, y = workgroup rows (ChzWg: up to 8 tiles of 8 channels, all of one source).
// A workgroup stages its source's window - bytes [2 M m0 - 2 Kp, 2 M (m0 + n)) of [history | this call], made signed -
// and the phasor table in LDS; each wave then owns one tile of 8 channels and walks the block in groups of 64 outputs
// (four 16-output MFMA tiles, two at a time: four independent accumulator chains):
//   MFMA   per 64-byte K-chunk q and tap plane p: acc[t][p] += A[q][p] x B[t][q], B read from the window (the window of
//          output j starts at byte 2 M (j + 1), 2-byte aligned for odd M: five dwords and v_alignbyte per operand)
//   VALU   A = lo + 256 hi, a = sat16((A + 128) >> 8), phasor from LDS, rotation on v_dot2_i32_i16, round / saturate,
//          byte pack into a per-wave LDS staging row of 8 channels x 128 bytes
//   store  one 16-byte store per lane: 8 lanes write one channel's 128 contiguous bytes (whole sectors)
// A second, tiny kernel writes each source's last Kp samples (the next call's history) with vector stores.
// The kernels of this file and of iqd_chan_{frac,survey,fmt,gain}.hip are put together from the pieces of iqd_chan_dev.h:
// here chz_walk<1, NQR, 1, CHZ_CONSECUTIVE> with ChzFinish and ChzRowSink<1, MAG> (MAG: the scan walker's squelch magnitude).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan.h"
#include "iqd_chan_dev.h"
#include "iqd_chains.h"

namespace iqd {

template <int NQR>   // NQR > 0: nq <= NQR, the A operands stay in registers; 0: they are read per group
__global__ __launch_bounds__(512) void chz_kernel(const ChzLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t chz_lds[];
    uint32_t *sp = (uint32_t *)chz_lds;
    uint8_t *stage_all = chz_lds + CHZ_PHASOR * 4;
    uint8_t *win = chz_lds + CHZ_LDS_FIXED;
    const uint32_t wave = threadIdx.x >> 6;
    const ChzWg w = a.wgs[blockIdx.y];
    const uint32_t m0 = blockIdx.x * a.t_blk;
    const uint32_t nloc = min(a.t_blk, a.n_out - m0);           // a multiple of 32

    chz_phasor_to_lds(a, sp);
    chz_stage_window<CHZ_U8>(a, w.source, m0, nloc, win);
    __syncthreads();
    if (wave >= w.n_tiles) return;

    ChzLaneTile<NQR> T;
    T.params(a, w.first_tile + wave, 1, true);
    T.load_a(a.nq);
    ChzRowSink<1, false> sink{stage_all + wave * (CHZ_TILE_CH * 2 * CHZ_GROUP), T.st_ch, 0};
    chz_walk<1, NQR, 1, CHZ_CONSECUTIVE>(a, win, 0, sp, T.A, T.amat, T.inc, m0, nloc, 0, 1, T.fin, sink);
}

// The scan walker (include/iqdemod.h: iqd_channelizer_follow_scanner).  One workgroup owns up to s.waves tiles of
// following channels of one source for the whole call and walks its blocks in order, s.wpt waves per tile (each takes
// every s.wpt-th group of 64 outputs of a window and keeps its own, identical, shadow copy); per block
//   1. the lane that owns a channel's shadow state (lane 8 l of the tile's wave for slot l) turns its current frequency
//      into the block's increment d_b, or into silence (out of band: zero taps, every output byte 0x80);
//   2. every lane builds its own part of the tile's A operands for d_b - exactly chz_pack_slot's bytes - from the
//      prototype and the phasor table in LDS (in registers for nq <= CHZ_NQ_REG, else in the tile's slice of a.amat);
//   3. the block's outputs go through chz_walk, window by window, summing the squelch magnitude;
//   4. the owner lanes step the shadow copy of their engine channel's per-block recurrence in squelch_track_kernel's
//      order: dBFS against the threshold with the IF gain in force, the tracker, scanner_step on a rejected block while
//      scanning, agc_run.
// The shadow state is dropped at the end: iqd_accept_iq_device on the rows re-derives the same decisions for real.
template <int NQR>
__global__ __launch_bounds__(512) void chz_scan_kernel(const ChzLaunch a, const ChzScanLaunch s)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t chz_lds[];
    uint32_t *sp = (uint32_t *)chz_lds;
    uint8_t *stage_all = chz_lds + CHZ_PHASOR * 4;
    int16_t *proto = (int16_t *)(chz_lds + CHZ_LDS_FIXED);
    uint32_t *magsum = (uint32_t *)(chz_lds + CHZ_LDS_FIXED + 2 * CHZ_PROTO_MAX);   // [2][CHZ_WAVES * 8], by block parity
    uint8_t *win = chz_lds + CHZ_LDS_FIXED + 2 * CHZ_PROTO_MAX + CHZ_SCAN_MAGSUM;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t tl = (tid >> 6) / s.wpt, part = (tid >> 6) % s.wpt;   // tile of the workgroup, share of its outputs
    const ChzWg w = a.wgs[blockIdx.x];
    const uint32_t kp = a.kp, nq = a.nq;

    chz_phasor_to_lds(a, sp);
    for (uint32_t i = tid; i < kp / 8; i += blockDim.x) ((uint4 *)proto)[i] = ((const uint4 *)s.proto)[i];

    const bool active = tl < w.n_tiles;
    const uint32_t tile = w.first_tile + (active ? tl : 0);
    ChzLaneTile<NQR> T;                                           // (its increments and A operands are built here, per block)
    T.params(a, tile, 1, active);
    const uint32_t col = lane & 15, g = lane >> 4, st_ch = T.st_ch;
    uint8_t *stage = stage_all + (tid >> 6) * (CHZ_TILE_CH * 2 * CHZ_GROUP);
    uint4 *amat = const_cast<uint4 *>(T.amat);
    const uint32_t a_slot = col >> 1, a_row = col & 1;           // the A rows this lane builds: slot a_slot, Ar / Ai
    const bool a_real = active && a.tiles[tile].ch[a_slot] != CHZ_NONE;

    // the shadow state, in the owner lane of each channel
    const bool owner = (lane & 7) == 0 && st_ch != CHZ_NONE;
    const uint32_t ech = s.first_ch + (owner ? st_ch : 0);
    AgcConfig cfg = s.agc_cfg[ech];
    AgcState st = s.agc[ech];
    const ScanConfig sc = s.scan_cfg[ech];
    ScanState ss = s.scan[ech];
    uint32_t gain = st.rx_gain, tracking = s.tracker[ech];
    const int32_t threshold = s.params[ech].threshold, rot = s.params[ech].rotation;
    const unsigned long long centre = s.centre[w.source];
    const Consts &cst = *s.consts;

    for (uint32_t b = 0; b < s.n_blocks; b++) {
        // 1. this block's increment, or silence
        uint32_t d = 0;
        const uint32_t on = owner && chz_tuning(a.m, centre, ss.current_hz, rot, &d) ? 1u : 0u;
#pragma unroll
        for (int i = 0; i < 2; i++) T.inc[i] = (uint32_t)__shfl((int)d, (int)(8 * (2 * g + i)));
        const uint32_t d_a = (uint32_t)__shfl((int)d, (int)(8 * a_slot));
        const uint32_t on_a = (uint32_t)__shfl((int)on, (int)(8 * a_slot));   // (every lane: the owner must be active)
        const bool live = a_real && on_a != 0;
        chz_block_open(magsum, b);
        // 2. A operands: K-index kappa = 64 q + 16 g + j is sample kp - 1 - kappa / 2, rail kappa & 1 (iqd_chan.h)
        __syncthreads();   // (the prototype; and the previous block's last window has been read)
        auto build = [&](uint32_t q, uint4 &vlo, uint4 &vhi) {
            uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
            if (live) {
#pragma unroll
                for (uint32_t j = 0; j < 8; j++) {
                    const uint32_t kk = kp - 1 - 32 * q - 8 * g - j;
                    const int32_t h = proto[kk];
                    const uint32_t p = sp[(kk * d_a) >> 20];
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
        };
        if (NQR > 0) {
#pragma unroll
            for (int q = 0; q < NQR; q++)
                if (q < (int)nq) {
                    uint4 vlo, vhi;
                    build((uint32_t)q, vlo, vhi);
                    T.A[q][0] = __builtin_bit_cast(chz_v4i, vlo);
                    T.A[q][1] = __builtin_bit_cast(chz_v4i, vhi);
                }
        } else if (active && part == 0) {   // one wave per tile writes them; the window's barrier comes before any read
            for (uint32_t q = 0; q < nq; q++) {
                uint4 vlo, vhi;
                build(q, vlo, vhi);
                amat[(q * 2 + 0) * 64] = vlo;
                amat[(q * 2 + 1) * 64] = vhi;
            }
        }
        // 3. the block's outputs, window by window
        ChzRowSink<1, true> sink{stage, st_ch, 0};
        const uint32_t mb = b * s.block_out, me = mb + s.block_out;
        for (uint32_t m0 = mb; m0 < me; m0 += s.t_blk) {
            const uint32_t nloc = min(s.t_blk, me - m0);
            if (m0 != mb) __syncthreads();
            chz_stage_window<CHZ_U8>(a, w.source, m0, nloc, win);
            __syncthreads();
            if (active) chz_walk<1, NQR, 1, CHZ_CONSECUTIVE>(a, win, 0, sp, T.A, amat, T.inc, m0, nloc, part, s.wpt, T.fin, sink);
        }
        // 4. the squelch's magnitude per channel, then the shadow step
        const uint32_t *ms = chz_block_close(magsum, b, tl, sink.mag, owner);
        if (owner) {
            const uint32_t avg = *ms / s.block_out;
            const int32_t dbfs = (int32_t)((uint32_t)magnitude_dbfs(cst, avg) - gain);
            const uint32_t present = dbfs >= threshold ? 1u : 0u;
            const uint32_t allowed = present | tracking;
            tracking = present;
            if (!allowed && sc.scanning) scanner_step(sc, ss);
            if (cfg.enabled) gain = agc_run(cst, cfg, st, avg, gain);
        }
    }
}

// the next call's history: the last 2 kp B raw bytes of [history | this call] per source
__global__ void chz_history_kernel(const ChzLaunch a)
{
    const uint32_t hb = 2 * a.kp * a.rail_bytes;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n_sources * hb) return;
    const uint32_t s = t / hb, i = t - s * hb;
    const int64_t b = (int64_t)a.bytes_per_source - hb + i;
    a.hist_next[t] = b < 0 ? a.hist[(size_t)s * hb + hb + b] : a.wide[(size_t)s * a.bytes_per_source + b];
}

hipError_t launch_channelizer_history(const ChzLaunch &a, hipStream_t st)
{
    const uint32_t nh = a.n_sources * 2 * a.kp * a.rail_bytes;
    hipLaunchKernelGGL(chz_history_kernel, dim3((nh + 255) / 256), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_channelizer(const ChzLaunch &a, uint32_t n_fixed_wgs, const ChzWg *scan_wgs, uint32_t n_scan_wgs,
                              const ChzScanLaunch *scan, hipStream_t st)
{
    const dim3 grid((a.n_out + a.t_blk - 1) / a.t_blk, n_fixed_wgs);
    const size_t lds = CHZ_LDS_FIXED + 2 * ((size_t)a.t_blk * a.m + a.kp) + 16;
    if (n_fixed_wgs) {
        if (a.den > 1) {
            hipError_t e = launch_channelizer_frac(a, n_fixed_wgs, st);   // (iqd_chan_frac.hip)
            if (e != hipSuccess) return e;
        } else if (a.nq <= CHZ_NQ_REG) hipLaunchKernelGGL(chz_kernel<CHZ_NQ_REG>, grid, dim3(512), lds, st, a);
        else hipLaunchKernelGGL(chz_kernel<0>, grid, dim3(512), lds, st, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (scan && n_scan_wgs) {
        const ChzScanLaunch &s = *scan;
        ChzLaunch b = a;
        b.wgs = scan_wgs;
        const size_t scan_lds = CHZ_LDS_FIXED + 2 * CHZ_PROTO_MAX + CHZ_SCAN_MAGSUM + 2 * ((size_t)s.t_blk * a.m + a.kp) + 16;
        const dim3 block(64 * s.waves * s.wpt);
        if (a.nq <= CHZ_NQ_REG) hipLaunchKernelGGL(chz_scan_kernel<CHZ_NQ_REG>, dim3(n_scan_wgs), block, scan_lds, st, b, s);
        else hipLaunchKernelGGL(chz_scan_kernel<0>, dim3(n_scan_wgs), block, scan_lds, st, b, s);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return launch_channelizer_history(a, st);
}

}  // namespace iqd
