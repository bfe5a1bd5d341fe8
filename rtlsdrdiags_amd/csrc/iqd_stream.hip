// WBFM chain as a streaming pipeline: one persistent 16-wave workgroup per CU (see iqd_stream.h).
// hipcc --offload-arch=gfx950 -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "iqd_kernels.h"
#include "iqd_stream.h"
#include "iqd_wbfm.h"
#include "iqd_mfma.h"
#include "iqd_stream_fix.h"
#include "iqd_taps.h"

namespace iqd {

// The IIR lanes' and the audio wave's 16-byte stores: a lane's PCM and the parts of its boundary record.
#define ST_STORE16(P, A, B, C, D) (*(u32x4 *)(P) = u32x4{A, B, C, D})


// The angle table starts at LDS address 0 (the kernel has no static LDS; checked when the kernel starts), so a table
// cell's byte offset IS its LDS address: through the generic `lds + offset` form the compiler adds the base - a
// relocated zero - to every one of the eight addresses of a piece.
typedef __attribute__((address_space(3))) const uint32_t lds_cu32;
__device__ __forceinline__ uint32_t st_table_read(uint32_t byte_offset) { return *(lds_cu32 *)(uintptr_t)byte_offset; }
// One 16-byte chunk of a ring slot, by its LDS address (the IIR lanes: st_iir_wave keeps the addresses).
typedef uint32_t st_u32v4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const st_u32v4 lds_cu32v4;
__device__ __forceinline__ u32x4 st_ring_read(uint32_t lds_address)
{
    const st_u32v4 v = *(lds_cu32v4 *)(uintptr_t)lds_address;   // (as one vector: one ds_read_b128)
    return u32x4{v.x, v.y, v.z, v.w};
}

#ifndef IQD_ST_WAITSTAT   // diagnostic build: how often each side of a ring sleeps on the other (per-wave counts, added once
#define IQD_ST_WAITSTAT 0 // per wave to ChainLaunch::stamps[0..3] = P sleeps, IIR sleeps, P pieces, IIR pieces; iqd_debug_stamps)
#endif

// How long a wave sleeps between two looks at its ring counter (units of 64 cycles).  A waiting wave's polls are
// instructions like any others, on a SIMD whose other waves are not waiting.
// s_sleep argument (x 64 cycles) between two looks at a ring counter.  A waiting wave's poll loop takes issue slots from the
// waves it waits for: with the counters read by ds_read_b32 (round 3: a flat_load before) one round of the loop is short, the
// waiters spun twice as often, and 8 % of the kernel's instructions were polls.  0.343 -> 0.332 ms from 1 / 1 to 6 / 10
// (3 / 3: 0.335, 10 / 10: 0.336, 16 / 16: 0.347, 24 / 24: 0.370).
#ifndef IQD_ST_SLEEP_P
#define IQD_ST_SLEEP_P 6
#endif
#ifndef IQD_ST_SLEEP_I
#define IQD_ST_SLEEP_I 10
#endif
#ifndef IQD_ST_SLEEP_A    // the audio wave waiting for a piece of a y2 ring
#define IQD_ST_SLEEP_A 10
#endif
// The IIR lanes' decimator taps: literals of the v_dot2c instructions (the designs are fixed, iqd_taps.h: STREAM_TAPS) instead of
// 30 scalar registers that the wave could not keep (85 of its scalar registers spilled to vector lanes, 14 v_readlane per piece).
#define ST_TAP(WHICH, Q) (uint32_t)taps::STREAM_TAPS.WHICH[Q]
#ifndef IQD_ST_TRACE      // diagnostic build: workgroup 5 writes clock64() of (hardware wave, piece, event k) to stamps[64 + ((wave * 256 + piece) * 4 + k)]
#define IQD_ST_TRACE 0
#endif
#if IQD_ST_TRACE
#define ST_TRACE(st, wave, piece, k) do { if (blockIdx.x == 5 && lane == 0 && (piece) < 256) (st)[64 + (((wave) * 256 + (int)(piece)) * 4 + (k))] = (unsigned long long)clock64(); } while (0)
#else
#define ST_TRACE(st, wave, piece, k) do { } while (0)
#endif
#ifndef IQD_ST_TIMING     // diagnostic build: where a P wave's and an IIR wave's cycles go, per SIMD (stamps[16 + 8 simd + k])
#define IQD_ST_TIMING 0
#endif
#if IQD_ST_TIMING
#define ST_T(var) const long long var = clock64()
__device__ __forceinline__ int st_simd_id() { return (__builtin_amdgcn_s_getreg((4 << 0) | (4 << 6) | (1 << 11)) ) & 3; }   // HW_ID[5:4]
#else
#define ST_T(var) do { } while (0)
#endif

// ---- P wave: 16 segments, raw bytes -> u[n] -------------------------------------------------------
// EPOCHS: some channel of the launch has a gain change whose samples a lead-in can still reach (GainEpochList; the host
// knows: iqd_set_gain).  The piecewise-gain lookup lives only in that instantiation - in the common one it would sit
// in the piece loop as a 16-deep ladder twice over, costing registers (it spilled) and instruction cache for nothing.
// GATED: a squelch-gated launch (some channel lost blocks): virtual sample v of a channel lives in its open block number
// v / block_samples (ChainLaunch::blk_lists); a lane keeps the block it is in and looks the next one up when it leaves it.
// BYGROUP: the launch holds channels of several rotation selectors (StreamArgs::grouped); this call takes the rounds in
// which the wave's 16 segments belong to selector ROT and leaves the others to the calls for the other two selectors
// (st_p_wave_any: +1, 0, -1 in turn - the order of the groups, so a wave still meets its rounds in ascending order).
// pc: pieces the wave's ring has seen so far, carried through those calls.
template <int ROT, bool MAG, bool EPOCHS, bool GATED, bool BYGROUP = false>
__device__ __forceinline__ void st_p_wave(const ChainLaunch &a, const StreamArgs &sa, uint8_t *lds, uint32_t *sync,
                                          int pw, int lane, uint32_t &pc)
{
    // a ring's four P waves are every third wave, not four in a row: the hardware issues oldest wave first, and with
    // rings of neighbouring waves ring 0 ran a third ahead of ring 2 (per-wave end times 115 / 137 / 155 us), which left
    // the last ring to finish on a nearly empty CU.  Now every ring has a wave of each age.
    const int cg = pw / ST_RINGS, ring = pw % ST_RINGS;
    if (ring >= (int)sa.rings) return;                           // (a workgroup of fewer rings: this wave's is not there)
    const uint32_t wg_segs = 64u * sa.rings;                     // segments per workgroup and round
    const int g = lane >> 4, c = lane & 15;
    const uint32_t row = (uint32_t)(16 * cg + c);                // ring row of this lane's segment
    uint8_t *ring_base = lds + ST_TABLE_BYTES + ring * (ST_RING_SLOTS * ST_SLOT_BYTES);
    const uint32_t *full = sync + ring * 8;        // [slot of the ring]: pieces written into it, x 4 P waves
    asm volatile("" : "+v"(full));                 // (the LDS address stays in a register: else a move per use)
    const uint32_t *consumed = full + 4;           // pieces the IIR wave has read (one register for both: an offset in the instruction)
    const uint32_t wr_off = st_slot_off(row, (uint32_t)g);
    const int src_lane4 = ((lane - 16) & 63) << 2;               // whose theta[3] precedes this lane's theta[0]

    v4i A[8];
#pragma unroll
    for (int m = 0; m < 8; m++) A[m] = ((const v4i *)(BYGROUP ? sa.amat3[1 - ROT] : sa.amat))[m * 64 + lane];
    v4i cbias = {WB_BIAS, WB_BIAS, WB_BIAS, WB_BIAS};
    const v4i czero = {0, 0, 0, 0};
    asm volatile("" : "+v"(cbias));  // four VGPRs for the whole kernel: else the compiler rebuilds the quad from scalars for every piece
    uint32_t zero = 0;
    asm volatile("" : "+v"(zero));   // a VGPR holding 0 for the SDWA negations

    const int n_pieces = (ST_HALO + (int)a.tile_len) >> 5;
    uint64_t inv_2pi = 0x3e22f9843e22f984ull;                    // (float)(1 / (2 pi)) twice: the scalar operand of v_pk_mul_f32
    asm volatile("" : "+s"(inv_2pi));
    for (uint32_t round = 0; round < sa.rounds; round++) {
        if ((round * chain_wgs(a) + chain_wg(a)) * wg_segs >= st_id_count(sa)) break;   // nothing left for this workgroup
        const uint32_t sid = (round * chain_wgs(a) + chain_wg(a)) * wg_segs + ring * 64 + row;
        int rot_of_id = ROT;
        const StSeg sg = BYGROUP ? st_segment_of(a, sa, sid, rot_of_id) : st_segment(a, sid, sa.n_segments);
        if (BYGROUP && __builtin_amdgcn_readfirstlane(rot_of_id) != ROT) continue;   // (uniform: groups are padded to 16 ids)
        const ChanParams &p = a.params[sg.ech];
        const uint8_t *iq_ch = a.iq + (size_t)sg.ch * a.ch_stride_bytes;
        const uint8_t *tail = a.tails + ((size_t)sg.ech * FAM_COUNT + FAM_WBFM) * TAIL_BYTES + TAIL_BYTES;
        const int32_t vmax = sg.vlen - 8;
        const float kneg = -p.wbfm_k;
        // segments whose lead-in reaches back before the call's start may meet earlier gains (GainEpochList)
        const GainEpochList *ep = &a.epochs[sg.ech].wbfm;
        const bool ep_reach = EPOCHS && ep->since[0] < (uint32_t)TAIL && (int64_t)sg.v0 - ST_HALO - 32 < -(int64_t)ep->since[0];
        const bool ep_any = EPOCHS && __any(ep_reach);
        // squelch magnitude bookkeeping, once per group of ST_AHEAD pieces: segments start on multiples of 128 samples of their
        // channel's stream, blocks and segment lengths are whole 128-sample units (iqd_create: block_bytes % 256 == 0; the
        // engine streams only rows of whole 128-sample units), so a group never straddles a block boundary or a segment's
        // end, and "inside the segment" is the same for the four lanes of a segment
        const int32_t mlim = MAG && sg.valid ? sg.tlen : INT32_MIN;   // groups at pos < mlim lie inside the segment
        uint32_t macc = 0;
        const uint32_t mblk0 = (uint32_t)sg.v0 / a.block_samples;
        uint32_t minblk = (uint32_t)sg.v0 - mblk0 * a.block_samples;
        uint32_t *mag_at = MAG ? a.mag_sums + (size_t)sg.ch * a.n_blocks + mblk0 : nullptr;   // the block's sum
        uint32_t gm16 = 0;                                       // the group's magnitudes, two 16-bit partial sums

        // this lane's 8 samples of the piece at `pos`: virtual sample v = v0 + 8 g + pos, from the kept tail while v < 0
        const int32_t vlane = sg.v0 + 8 * g;
        const uint8_t *base_iq = iq_ch + 2 * (int64_t)vlane, *base_tail = tail + 2 * (int64_t)vlane;
        const int32_t pos_max = vmax - vlane;
        const uint32_t *blk_list = GATED ? a.blk_lists + (size_t)sg.ch * a.n_blocks : nullptr;
        int32_t gb_v0 = 0, gb_v1 = 0;                            // GATED: virtual range of the open block this lane is in
        const uint8_t *gb_base = iq_ch;                          // ... and the address its virtual sample 0 would have
        auto piece_address = [&](int pos) -> const uint8_t * {
            const int32_t pc = pos < pos_max ? pos : pos_max;
            if (!GATED) {
                const uint8_t *base = pc < -vlane ? base_tail : base_iq;
                return base + 2 * (int64_t)pc;
            }
            const int32_t vv = vlane + pc;
            if (vv >= 0 && (vv >= gb_v1 || vv < gb_v0)) {        // (rare) into another open block
                const uint32_t blk = (uint32_t)vv / a.block_samples;
                gb_v0 = (int32_t)(blk * a.block_samples);
                gb_v1 = gb_v0 + (int32_t)a.block_samples;
                gb_base = iq_ch + 2 * ((int64_t)blk_list[blk] * a.block_samples - (int64_t)gb_v0);
            }
            return vv < 0 ? base_tail + 2 * (int64_t)pc : gb_base + 2 * (int64_t)vv;
        };
        // ST_AHEAD pieces of input in flight per wave (a piece's arithmetic is about as long as a trip to HBM under load:
        // with one piece asked for in advance the wave stood at the loop's head waiting - and 12 waves x 1 KB in flight per
        // CU cap the chip near 1.5 TB/s whatever the arithmetic costs).  The loads are the untracked ones of iqd_mfma.h:
        // the compiler's own wait placement would join the loop's back edge to vmcnt(0).  A buffer is re-asked right after
        // the last use of its old contents, in ST_AHEAD copies of the loop body with named buffers.
        // Not GATED: the piece to ask for next advances by 64 bytes per piece and is held at the last piece that lies wholly
        // inside the channel's samples (what is computed from a repeated piece lies beyond the segment's end and is never
        // stored or counted), and moves from the kept tail to the call's own samples when a first segment's lead-in ends
        // (below, once per segment) - instead of piece_address()'s six operations per piece.  Its address is
        // `nxt` + min(2 (position - ST_NXT_ORIGIN), nxt_max): the position is the same in all lanes, a scalar, so a piece pays
        // one v_min_u32 and the 64-bit add of the load's address.  `nxt` is piece_address() of the first request; a lane
        // whose samples end before that one (pos_last < ST_NXT_ORIGIN) stays there: nxt_max = 0.
        const int32_t pos_last = pos_max & ~31;
        const bool from_tail = sg.v0 == 0;                       // (tile_len >= ST_MIN_TILE = ST_HALO: only a first segment's lead-in reads the tail inside the loop)
        const uint8_t *nxt = piece_address(-ST_HALO + 32 * ST_AHEAD);
        constexpr int ST_NXT_ORIGIN = -ST_HALO + 32 * ST_AHEAD;
        auto nxt_room = [&](int32_t from) -> uint32_t {   // bytes from position `from` to the last whole piece, 0 if it lies before
            const int64_t room = 2 * ((int64_t)pos_last - from);
            return room < 0 ? 0u : room > 0x7fffff00 ? 0x7fffff00u : (uint32_t)room;
        };
        uint32_t nxt_max = nxt_room(ST_NXT_ORIGIN);
        uint4 prev = st_front<ROT>(*(const uint4 *)piece_address(-ST_HALO - 32), zero);
        v4u raw[ST_AHEAD];
#pragma unroll
        for (int j = 0; j < ST_AHEAD; j++) raw[j] = gload16_untracked(piece_address(-ST_HALO + 32 * j));
        // theta' of the sample before the lead-in (a warm segment's carried state applies from the lead-in's very first
        // sample, whose delta theta needs it): the last output of the piece before, from that piece's "N" window
        float last_prev;                                         // theta'[3] of this lane's previous window
        {
            const v4i bn = v4i{(int)prev.x, (int)prev.y, (int)prev.z, (int)prev.w};
            const v4i ilo = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[0], bn, cbias, 0, 0, 0);
            const v4i ihi = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[1], bn, czero, 0, 0, 0);
            const v4i qlo = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[2], bn, cbias, 0, 0, 0);
            const v4i qhi = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[3], bn, czero, 0, 0, 0);
            const uint32_t ti = (uint32_t)ilo[3] + ((uint32_t)ihi[3] << 8), tq = (uint32_t)qlo[3] + ((uint32_t)qhi[3] << 8);
            // Only row 3 of the four results is used.  Left to itself the allocator hands the twelve dead registers out again
            // at once - in the squelch-gated instantiations to an UNTRACKED load issued right behind the matrix instruction,
            // which the compiler does not guard against the matrix unit's pending write (tools/isa_lint.py: lint_mfma_readers;
            // benign in practice, the load's bytes arrive long after, but not by construction).  Kept alive until the
            // compiler's own first use above has waited for the results.
            asm volatile("" :: "v"(ilo), "v"(ihi), "v"(qlo), "v"(qhi), "v"(ti), "v"(tq));
            uint32_t rr;
            asm("v_msad_u8 %0, %1, %2, 0" : "=v"(rr) : "v"(tq), "s"(0x00800000u));
            const uint32_t t = st_table_read(rr * (uint32_t)(ST_ROW_FLOATS * 4) + (bfe(ti, 16, 8) << 2));
            last_prev = u2f((t & 0x7fffffffu) | ((tq << 8) & 0x80000000u));
        }
        // one piece: `prev` = the signed bytes of the piece before, `cur` = this piece's (output).  The loop below runs two
        // copies of the body with the two buffers swapped, so that neither is ever copied.
        uint32_t n_sleeps = 0;                                   // (IQD_ST_WAITSTAT)
#if IQD_ST_TIMING
        long long tt[4] = {0, 0, 0, 0};
#endif
        auto do_piece = [&](const int q, const int j, const uint4 &prev, uint4 &cur) __attribute__((always_inline)) {
            const int pos = -ST_HALO + 32 * q;
            ST_TRACE(a.stamps, pw + 3, q, 0);
            ST_T(t0);
            gload_wait<ST_AHEAD - 1>(raw[j]);                    // younger than this buffer's load: the other buffers' loads
            ST_T(t1);
            const uint4 raw_cur = as_uint4(raw[j]);              // (offset binary, as loaded: the squelch magnitudes below)
            cur = st_front<ROT>(raw_cur, zero);
            // both windows' MFMAs go out first: the second window's run under the first window's index arithmetic.
            // "S" window (the piece's first 16 outputs): lanes 0-31 this piece's first 32 bytes, lanes 32-63 the
            // previous piece's last 32; "N" window: the piece itself.
            const v4i bs = v4i{(int)(lane < 32 ? cur.x : prev.x), (int)(lane < 32 ? cur.y : prev.y),
                               (int)(lane < 32 ? cur.z : prev.z), (int)(lane < 32 ? cur.w : prev.w)};
            const v4i bn = v4i{(int)cur.x, (int)cur.y, (int)cur.z, (int)cur.w};
            v4i acc[2][4];
            acc[0][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[4], bs, cbias, 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[5], bs, czero, 0, 0, 0);
            acc[0][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[6], bs, cbias, 0, 0, 0);
            acc[0][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[7], bs, czero, 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[0], bn, cbias, 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[1], bn, czero, 0, 0, 0);
            acc[1][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[2], bn, cbias, 0, 0, 0);
            acc[1][3] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[3], bn, czero, 0, 0, 0);
            // phase A, both windows: table addresses and the gathers.  Twice the Q15 sums + WB_BIAS: byte 2 is
            // (uint8)((int8)(acc >> 15) + 128), the table index.
            uint32_t traw[2][4], tqs[2][4];
#pragma unroll
            for (int half = 0; half < 2; half++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const uint32_t ti = (uint32_t)acc[half][0][r] + ((uint32_t)acc[half][1][r] << 8);
                    const uint32_t tq = (uint32_t)acc[half][2][r] + ((uint32_t)acc[half][3][r] << 8);
                    uint32_t rr;                                 // |y| = |byte 2 of tq - 128|
                    asm("v_msad_u8 %0, %1, %2, 0" : "=v"(rr) : "v"(tq), "s"(0x00800000u));
                    const uint32_t x4 = bfe(ti, 16, 8) << 2;
                    uint32_t addr;                               // row |y|, column x of the half table
                    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(addr) : "v"(rr), "s"((uint32_t)(ST_ROW_FLOATS * 4)), "v"(x4));
                    traw[half][r] = st_table_read(addr);
                    tqs[half][r] = tq;
                }
            }
            uint32_t seen = lds_load_relaxed(consumed);          // asked early, needed only before the ring stores
            // phase B: squelch magnitudes of this lane's 8 samples, while the gathers are in flight (two packed 16-bit sums,
            // folded and booked once per group of pieces: at most 4 x 4 x 192 per half)
            if (MAG && pos >= 0) gm16 = st_mag_raw_chunk(raw_cur, gm16);
            // (after the last use of the buffer's old contents)
            if (GATED) {
                raw[j] = gload16_untracked(piece_address(pos + 32 * ST_AHEAD));
            } else {
                const uint32_t at = (uint32_t)(2 * (pos + 32 * ST_AHEAD - ST_NXT_ORIGIN));   // (uniform)
                raw[j] = gload16_untracked(nxt + (at < nxt_max ? at : nxt_max));
            }
            // phase C, both windows: sign, delta theta, branch cut, K, b0.  A window's angles are kept as the ALIGNED register
            // pairs X = (theta0, theta2), Y = (before, theta1), Z = (theta1, theta3): (d0, d2) = X - Y and (d1, d3) = Z - X are
            // then two packed subtractions of pairs as they stand.  Pairs of neighbours - (before, theta0) with (theta0, theta1) -
            // put theta0 and theta2 into two pairs at different halves: four register moves per piece.  Here only theta1 sits
            // in two pairs, and its v_bfi_b32 is simply issued twice.  The ring chunk holds (u0, u2, u1, u3): st_iir_piece, st_iir_lead_in.
            v2f u[2][2];
#pragma unroll
            for (int half = 0; half < 2; half++) {
                const int wpos = pos + 16 * half;
                uint32_t th[4], th1_z;          // the table holds |theta|; theta' = -theta carries the sign bit of y >= 0 (index bit 7)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(th[r]) : "s"(0x7fffffffu), "v"(traw[half][r]), "v"(tqs[half][r] << 8));
                // (another text: two identical statements are one to the compiler, and the copy comes back)
                asm("v_bfi_b32 %0, %1, %2, %3 ; theta1 of the pair Z" : "=v"(th1_z) : "s"(0x7fffffffu), "v"(traw[half][1]), "v"(tqs[half][1] << 8));
                const float give = g == 3 ? last_prev : u2f(th[3]);
                const float before = u2f((uint32_t)__builtin_amdgcn_ds_bpermute(src_lane4, (int)f2u(give)));
                last_prev = u2f(th[3]);
                float kk = kneg;
                if (EPOCHS && ep_any && ep_reach) kk = -epoch_gain_search(ep, p.wbfm_k, sg.v0 + wpos);   // (rare: right after a gain change)
                const v2f X = {u2f(th[0]), u2f(th[2])}, Y = {before, u2f(th[1])}, Z = {u2f(th1_z), u2f(th[3])};
#pragma unroll
                for (int e = 0; e < 2; e++) {   // two samples per packed operation; wrap_delta() of iqd_prims.h operation by operation
                    v2f d = e == 0 ? X - Y : Z - X;   // = -(delta theta) of samples (0, 2), then (1, 3)
                    v2f m = pk_mul_s(d, inv_2pi);
                    m.x = __builtin_rintf(m.x);
                    m.y = __builtin_rintf(m.y);
                    d = __builtin_elementwise_fma(-m, v2f{6.28318548202514648f, 6.28318548202514648f}, d);
                    d = __builtin_elementwise_fma(-m, v2f{-1.74845553146951715e-7f, -1.74845553146951715e-7f}, d);
                    const v2f v = d * v2f{kk, kk};
                    u[half][e] = v2f{sa.b0, sa.b0} * v;
                }
            }
            // hand the 2 x 4 samples to the IIR wave: the ring's two slots hold one piece (window 0, window 1), free once
            // the IIR wave has read the previous piece.  One signal per piece in each direction.
            ST_T(t2);
            ST_TRACE(a.stamps, pw + 3, q, 1);
            // (the counter is one LDS word, the same in every lane: one v_readfirstlane_b32 and the test runs on the scalar unit)
            seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)seen);
            while ((int32_t)(seen + (uint32_t)(ST_DEPTH - 1) - pc) < 0) {   // piece pc - ST_DEPTH has been read: its slots are free
                __builtin_amdgcn_s_sleep(IQD_ST_SLEEP_P);
                seen = lds_load_relaxed(consumed);
                seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)seen);
                if (IQD_ST_WAITSTAT) n_sleeps++;
            }
            ST_T(t3);
            ST_TRACE(a.stamps, pw + 3, q, 2);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            uint8_t *const slot = ring_base + (ST_DEPTH > 1 ? (pc & (uint32_t)(ST_DEPTH - 1)) * (2 * ST_SLOT_BYTES) : 0u) + wr_off;
            *(u32x4 *)slot = u32x4{f2u(u[0][0].x), f2u(u[0][0].y), f2u(u[0][1].x), f2u(u[0][1].y)};
            *(u32x4 *)(slot + ST_SLOT_BYTES) = u32x4{f2u(u[1][0].x), f2u(u[1][0].y), f2u(u[1][1].x), f2u(u[1][1].y)};
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            lds_signal(ST_DEPTH > 1 ? full + (pc & (uint32_t)(ST_DEPTH - 1)) : full);
            ST_TRACE(a.stamps, pw + 3, q, 3);
            pc++;
#if IQD_ST_TIMING
            { ST_T(t4); tt[0] += t1 - t0; tt[1] += t2 - t1; tt[2] += t3 - t2; tt[3] += t4 - t3; }
#endif
        };
        uint4 other;
        // The groups in two runs of one loop: the lead-in's up to the last request for a sample before position 0, then the
        // rest.  Between them - a scalar branch, once per segment - a first segment's requests move from the kept tail to the
        // call's own samples.
        const int q_samples = !GATED ? ST_HALO / 32 - ST_AHEAD : n_pieces;   // (n_pieces >= ST_HALO / 16)
        int q = 0;
#pragma unroll 1
        for (int q_end = q_samples; q < n_pieces; q_end = n_pieces) {
            for (; q < q_end; q += ST_AHEAD) {   // (n_pieces is a multiple of 4)
#pragma unroll
                for (int j = 0; j < ST_AHEAD; j += 2) {
                    do_piece(q + j, j, prev, other);
                    do_piece(q + j + 1, j + 1, other, prev);
                }
                const int gpos = -ST_HALO + 32 * q;                  // the group's first sample
                if (MAG && gpos >= 0) {
                    const uint32_t m = (gm16 & 0xffffu) + (gm16 >> 16);
                    gm16 = 0;
                    macc += gpos < mlim ? m : 0u;
                    minblk += 32 * ST_AHEAD;
                    if (minblk >= a.block_samples) {                 // the next group belongs to the next block
                        if (macc) atomicAdd(mag_at, macc);
                        macc = 0;
                        mag_at++;
                        minblk -= a.block_samples;
                    }
                }
            }
            if (!GATED && q == q_samples && from_tail) {   // the next piece asked for is the one at position 0
                nxt = (const uint8_t *)((uintptr_t)(a.iq + (size_t)sg.ch * a.ch_stride_bytes + 16 * g) + (intptr_t)(2 * ST_NXT_ORIGIN));
                nxt_max = nxt_room(0) + (uint32_t)(-2 * ST_NXT_ORIGIN);
            }
        }
#pragma unroll
        for (int j = 0; j < ST_AHEAD; j++) gload_wait<0>(raw[j]);   // the loads asked for beyond the last piece: drained before their registers move on
        if (MAG && macc) atomicAdd(mag_at, macc);
        if (IQD_ST_WAITSTAT && lane == 0) {
            atomicAdd(&a.stamps[0], (unsigned long long)n_sleeps);
            atomicAdd(&a.stamps[2], (unsigned long long)n_pieces);
        }
#if IQD_ST_TIMING
        if (lane == 0) {   // per P wave of the workgroup: [16 + pw] compute, [32 + pw] ring wait, [48 + pw] raw wait + hand-over
            atomicAdd(&a.stamps[16 + pw], (unsigned long long)tt[1]);
            atomicAdd(&a.stamps[32 + pw], (unsigned long long)tt[2]);
            atomicAdd(&a.stamps[48 + pw], (unsigned long long)(tt[0] + tt[3]));
        }
#endif
    }
}

// ---- IIR wave: 64 segments, u[n] -> pairs of stage-2 outputs for the audio wave -----------------------
struct StIir {
    float y, up;
    uint32_t wlast[2];     // the last 4 (int16)y
    uint32_t wq0[2];       // the first 4 (int16)y of the window just processed
    uint32_t y1h[4];       // the last 8 stage-1 outputs
    uint32_t y2lo;         // first stage-2 output of the current piece
    uint32_t n_sleeps;     // (IQD_ST_WAITSTAT)
    int ring;              // (IQD_ST_TRACE)
    unsigned long long *stamps;
#if IQD_ST_TIMING
    long long t_wait, t_seen, t_to_consumed;
#endif
};

// The de-emphasis filter's input sums t[n] = u[n] + u[n-1] of one window, from its four ring chunks (u0, u2, u1, u3) and the sample
// before.  (t1, t3) = (u1, u3) + (u0, u2) is ONE packed addition of the two register pairs as ds_read_b128 delivers them - the same
// IEEE addition per element, and off the recurrence's chain; t2 = u2 + u1 and t0 = u0 + (u3 of the chunk before) are single ones.
__device__ __forceinline__ void st_iir_sums(const u32x4 (&v)[4], float up, float (&sum)[16])
{
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const float u0 = u2f(v[g].x), u2 = u2f(v[g].y), u1 = u2f(v[g].z), u3 = u2f(v[g].w);
        sum[4 * g] = u0 + up;
        const v2f t13 = v2f{u1, u3} + v2f{u0, u2};
        sum[4 * g + 1] = t13.x;
        sum[4 * g + 3] = t13.y;
        sum[4 * g + 2] = u2 + u1;
        up = u3;
    }
}

// 16 samples of one segment: de-emphasis (IirFilter.cc:161-176 op by op), (int16), /4 with 8 taps, then one
// /4 output with 12 taps.  Returns that stage-2 output.
__device__ __forceinline__ int st_iir_window(const StreamArgs &sa, StIir &s, const u32x4 (&v)[4], int c14, int c15)
{
    uint32_t wq[10];                                   // 20 samples: the last quad, then this window's four
    float y = s.y;
    const float a1 = sa.a1;
    float sum[16];
    st_iir_sums(v, s.up, sum);
#pragma unroll
    for (int k = 0; k < 8; k++) {                      // (IQD_IIR_STEP with its sum formed ahead: r = a1 y, y = t - r)
        y = sum[2 * k] - a1 * y;
        const float y_even = y;
        y = sum[2 * k + 1] - a1 * y;
        wq[2 + k] = cast_pack_i16_bounded(y_even, y);
    }
    const float up = u2f(v[3].w);
    s.y = y;
    s.up = up;
    wq[0] = s.wlast[0];
    wq[1] = s.wlast[1];
    s.wlast[0] = wq[8];
    s.wlast[1] = wq[9];
    s.wq0[0] = wq[2];
    s.wq0[1] = wq[3];
    // stage 1 with DOUBLED taps (|2 h| <= 12892 fits int16; the sums stay below 2^31: 2 (16384 + 29126 * 32768)): the
    // output (acc >> 15) then sits in the high half of the accumulator and two of them pack with one v_perm_b32, no shifts.
    // The accumulators start from a register holding the rounding term (c15 = 1 << 15, c14 = 1 << 14): as constants the
    // compiler re-materialises them with a move in front of every chain.
    uint32_t y1[4];
#pragma unroll
    for (int o = 0; o < 4; o++) {                      // window x[4m-4 .. 4m+3] <-> taps h[7 .. 0]
        int acc = dot2_from(wq[2 * o], sa.d1p2[0], c15);
        acc = dot2(wq[2 * o + 1], ST_TAP(d1p2, 1), acc);
        acc = dot2(wq[2 * o + 2], ST_TAP(d1p2, 2), acc);
        acc = dot2(wq[2 * o + 3], ST_TAP(d1p2, 3), acc);
        y1[o] = (uint32_t)acc;
    }
    // stage 2: output k from y1[4k-8 .. 4k+3], 12 taps, newest pair first
    const uint32_t d[6] = {s.y1h[0], s.y1h[1], s.y1h[2], s.y1h[3], pack_hi16(y1[0], y1[1]), pack_hi16(y1[2], y1[3])};
    int acc = dot2_from(d[5], sa.p12p[0], c14);
#pragma unroll
    for (int q = 1; q < 6; q++) acc = dot2(d[5 - q], ST_TAP(p12p, q), acc);
    s.y1h[0] = d[2];
    s.y1h[1] = d[3];
    s.y1h[2] = d[4];
    s.y1h[3] = d[5];
    return acc >> 15;
}

struct StIirSeg {
    StSeg sg;
    int32_t back;          // tile 0: the carried exact state sits `back` samples before the tile; else -1
    float cy_y, cy_u;
    int32_t rec_pos;
    WbfmRecord rec;
    StHist *hist;          // this segment's boundary record
    int c14, c15;          // 1 << 14, 1 << 15 in registers (the decimators' rounding terms)
};

// Whether a ring takes the IIR wave's fast path, from what each of its 64 lanes knows about its segment (not there at all, or
// cold, of full length and not the keeper of its channel's restart state).  The IIR wave and the audio wave both ask: a fast ring
// hands its first pair over at position 0, any other from the lead-in's first piece on.
__device__ __forceinline__ bool st_ring_is_fast(uint32_t valid, int32_t back, int32_t tlen, uint32_t tile_len, bool keeps_restart)
{
    return __all(!valid || (back < 0 && tlen == (int32_t)tile_len && !keeps_restart)) != 0;
}

// The y2 ring of one IIR ring as a lane sees it: its dword of slot 0 and the two counters (iqd_stream.h: st_y2_piece).
struct StY2Ring {
    uint8_t *lane_slot0;
    const uint32_t *full, *consumed;
};
__device__ __forceinline__ StY2Ring st_y2_ring(uint8_t *lds, uint32_t *sync, int ring, int lane)
{
    return StY2Ring{lds + ST_Y2_OFF + ring * ST_Y2_RING_BYTES + lane * 4, sync + ring * 8 + ST_SYNC_Y2_FULL, sync + ring * 8 + ST_SYNC_Y2_CONSUMED};
}

// (q.sg.valid bit 1: the segment keeps the channel's restart state - WbfmRecord::pad - at q.rec_pos, and takes its own record
//  where every full cold segment does, rec_pos_uniform)
__device__ __forceinline__ void st_iir_marks(const ChainLaunch &a, StIirSeg &q, StIir &s, int pos, int rec_pos_uniform)
{
    if (q.back >= 0) {                                 // warm segment: silence before the carried state applies
        if (pos == -q.back) { s.y = q.cy_y; s.up = q.cy_u; }
        else if (pos < -q.back) { s.y = 0.f; s.up = 0.f; }
    } else if (pos == 0) {                             // cold segment: the warmed-up state, checked against the predecessor's end
        q.rec.y_in = s.y;
    }
    if (pos == q.rec_pos) {
        if (q.sg.valid & 2u) {   // (parked in the spare words of the segment's boundary record, whose address is at hand: no register for it)
            q.hist->pad[0] = f2u(s.y);
            q.hist->pad[1] = f2u(s.up);
        } else {
            q.rec.y_out = s.y;
            q.rec.u_out = s.up;
        }
    }
    if ((q.sg.valid & 2u) && pos == rec_pos_uniform) { q.rec.y_out = s.y; q.rec.u_out = s.up; }
    if (pos == q.sg.tlen) {                            // (the last 40 stage-2 outputs are the audio wave's to store: st_audio_wave)
        q.rec.y_end = s.y;
        q.rec.u_end = s.up;
        if (q.sg.valid) {
            ST_STORE16(q.hist->y1_last, s.y1h[0], s.y1h[1], s.y1h[2], s.y1h[3]);
            *(u32x2 *)q.hist->w_last = u32x2{s.wlast[0], s.wlast[1]};
        }
    }
}

// FAST: every segment of the wave is cold and of full length (or not there at all), so the few things that happen at
// particular positions happen at the SAME position in every lane - one scalar compare per window instead of a dozen
// per-lane compare-and-select operations - and the lead-in has already been run by st_iir_lead_in().
// sync_a: the LDS byte address of the ring's sync words, in a vector register (lds_word_uniform).
// yk: pieces this wave has handed to the audio wave so far (all rounds).
template <bool FAST>
__device__ __forceinline__ void st_iir_piece(const ChainLaunch &a, const StreamArgs &sa, const uint32_t (&rd_a)[4], uint32_t sync_a,
                                             uint32_t &wg, const StY2Ring &y2r, uint32_t &yk, StIirSeg &q, StIir &s, int pos, int lane,
                                             int rec_pos_uniform)
{
    uint32_t y2_seen = 0;
#pragma unroll
    for (int half = 0; half < 2; half++) {
        const int wpos = pos + 16 * half;
        if (half == 0) {   // the four P waves of the ring have written piece `wg` (both windows) when `full` reaches 4 (wg + 1)
            const uint32_t target = 4u * (wg / (uint32_t)ST_DEPTH + 1u);
            const uint32_t full_off = ST_DEPTH > 1 ? 4u * (wg & (uint32_t)(ST_DEPTH - 1)) : 0u;
            ST_T(tw0);
            uint32_t seen = lds_word_uniform(sync_a, full_off);
            while ((int32_t)(seen - target) < 0) {
                __builtin_amdgcn_s_sleep(IQD_ST_SLEEP_I);
                seen = lds_word_uniform(sync_a, full_off);
                if (IQD_ST_WAITSTAT) s.n_sleeps++;
            }
#if IQD_ST_TIMING
            { ST_T(tw1); s.t_wait += tw1 - tw0; s.t_seen = tw1; }
#endif
            ST_TRACE(s.stamps, s.ring, wg, 0);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        const uint32_t slot = (ST_DEPTH > 1 ? (wg & (uint32_t)(ST_DEPTH - 1)) * (2 * ST_SLOT_BYTES) : 0u) + half * ST_SLOT_BYTES;
        u32x4 v[4];                                    // a chunk holds (u0, u2, u1, u3): st_p_wave, phase C
#pragma unroll
        for (int gq = 0; gq < 4; gq++) v[gq] = st_ring_read(rd_a[gq] + slot);
        if (half == 1) {   // both windows read: the ring is free for the next piece
            // asked early (it returns with the reads above), needed only before the hand-over
            y2_seen = lds_load_relaxed((const uint32_t *)(uintptr_t)(sync_a + 4u * ST_SYNC_Y2_CONSUMED));
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the reads have returned
            lds_signal_at<16>(sync_a);
            ST_TRACE(s.stamps, s.ring, wg, 1);
            wg++;
#if IQD_ST_TIMING
            { ST_T(tc); s.t_to_consumed += tc - s.t_seen; }
#endif
        }
        if (!FAST) st_iir_marks(a, q, s, wpos, rec_pos_uniform);
        else if (wpos == rec_pos_uniform) { q.rec.y_out = s.y; q.rec.u_out = s.up; }
        const int y2 = st_iir_window(sa, s, v, q.c14, q.c15);
        if (wpos >= 0 && wpos < 48 && q.sg.valid) {    // (uniform) the segment's first values, for the boundary fix-up
            if (wpos == 0) ST_STORE16(q.hist->w_first, s.wq0[0], s.wq0[1], s.y1h[2], s.y1h[3]);   // (w_first, y1_first[0..1])
            else *(u32x2 *)&q.hist->y1_first[wpos >> 3] = u32x2{s.y1h[2], s.y1h[3]};
        }
        if (half == 0) s.y2lo = (uint32_t)y2;
        else {   // the piece's pair goes to the audio wave: its slot is free once piece yk - ST_Y2_DEPTH has been read
            const StY2Piece yp = st_y2_piece(yk, ST_Y2_DEPTH, ST_Y2_EVERY);
            // (one LDS word, the same in every lane: the test runs on the scalar unit)
            y2_seen = (uint32_t)__builtin_amdgcn_readfirstlane((int)y2_seen);
            while ((int32_t)(y2_seen - yp.need_consumed) < 0) {
                __builtin_amdgcn_s_sleep(IQD_ST_SLEEP_I);
                y2_seen = lds_word_uniform(sync_a, 4u * ST_SYNC_Y2_CONSUMED);
                if (IQD_ST_WAITSTAT) s.n_sleeps++;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            *(uint32_t *)(y2r.lane_slot0 + yp.slot * ST_Y2_SLOT_BYTES) = pack_lo16(s.y2lo, (uint32_t)y2);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if (yp.add_full) lds_signal_at<4 * ST_SYNC_Y2_FULL>(sync_a, yp.add_full);
            yk++;
        }
    }
    ST_TRACE(s.stamps, s.ring, wg - 1, 2);
}

// The lead-in of a wave whose segments are all cold: only the de-emphasis recurrence (its state is what the lead-in is
// for; a cold segment's decimators start with histories that the boundary fix-up replaces anyway).
__device__ __forceinline__ void st_iir_lead_in(const StreamArgs &sa, const uint32_t (&rd_a)[4], uint32_t sync_a,
                                               uint32_t &wg, StIir &s)
{
    float y = s.y, up = s.up;
    const float a1 = sa.a1;
    for (int piece = 0; piece < ST_HALO / 32; piece++) {
        const uint32_t target = 4u * (wg / (uint32_t)ST_DEPTH + 1u);
        const uint32_t full_off = ST_DEPTH > 1 ? 4u * (wg & (uint32_t)(ST_DEPTH - 1)) : 0u;
        uint32_t seen = lds_word_uniform(sync_a, full_off);
        while ((int32_t)(seen - target) < 0) {
            __builtin_amdgcn_s_sleep(IQD_ST_SLEEP_I);
            seen = lds_word_uniform(sync_a, full_off);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        u32x4 v[2][4];
#pragma unroll
        for (int half = 0; half < 2; half++)
#pragma unroll
            for (int gq = 0; gq < 4; gq++)
                v[half][gq] = st_ring_read(rd_a[gq] + (ST_DEPTH > 1 ? (wg & (uint32_t)(ST_DEPTH - 1)) * (2 * ST_SLOT_BYTES) : 0u) + half * ST_SLOT_BYTES);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the reads have returned
        lds_signal_at<16>(sync_a);
        wg++;
#pragma unroll
        for (int half = 0; half < 2; half++) {
            float sum[16];
            st_iir_sums(v[half], up, sum);
#pragma unroll
            for (int k = 0; k < 16; k++) y = sum[k] - a1 * y;
            up = u2f(v[half][3].w);
        }
    }
    s.y = y;
    s.up = up;
}

__device__ __forceinline__ void st_iir_wave(const ChainLaunch &a, const StreamArgs &sa, uint8_t *lds, uint32_t *sync,
                                            int ring, int lane)
{
    uint8_t *ring_base = lds + ST_TABLE_BYTES + ring * (ST_RING_SLOTS * ST_SLOT_BYTES);
    const StY2Ring y2r = st_y2_ring(lds, sync, ring, lane);
    // the ring's sync words ([0 .. 3] `full`, [4] `consumed`, [5], [6] the y2 ring's): their LDS address lives in a vector register
    // for the wave's whole life, and every look at one of them is that register plus a constant (lds_word_uniform)
    uint32_t sync_a = (uint32_t)(uintptr_t)(sync + ring * 8);
    asm volatile("" : "+v"(sync_a));
    // the LDS byte addresses of the lane's four chunks of the ring's first slot (st_slot_off), in four vector registers for the wave's
    // whole life: every ring read is one of them plus a constant
    uint32_t rd_a[4];
#pragma unroll
    for (int gq = 0; gq < 4; gq++) {
        rd_a[gq] = (uint32_t)(uintptr_t)ring_base + st_slot_off((uint32_t)lane, (uint32_t)gq);
        asm volatile("" : "+v"(rd_a[gq]));
    }
    const int n_pieces = (ST_HALO + (int)a.tile_len) >> 5;       // a multiple of 4
    if (ring >= (int)sa.rings) return;
    const uint32_t wg_segs = 64u * sa.rings;
    uint32_t wg = 0;                                             // pieces read so far (all rounds)
    uint32_t yk = 0;                                             // pieces handed to the audio wave so far (all rounds)
    for (uint32_t round = 0; round < sa.rounds; round++) {
        if ((round * chain_wgs(a) + chain_wg(a)) * wg_segs >= st_id_count(sa)) break;
        const uint32_t sid = (round * chain_wgs(a) + chain_wg(a)) * wg_segs + ring * 64 + lane;
        StIirSeg q;
        int rot_unused;
        q.sg = st_segment_of(a, sa, sid, rot_unused);
        q.hist = sa.hist + (q.sg.valid ? (size_t)q.sg.li * a.tiles_per_ch + q.sg.tile : 0);
        q.back = -1;
        q.cy_y = q.cy_u = 0.f;
        q.c14 = 1 << 14;
        q.c15 = 1 << 15;
        asm volatile("" : "+v"(q.c14), "+v"(q.c15));
        int32_t carried_back = ST_HALO;
        if (q.sg.tile == 0) {
            const WbfmCarry cy = a.wbfm_carry[q.sg.ech];
            q.back = cy.back;
            q.cy_y = cy.y;
            q.cy_u = cy.u;
            carried_back = cy.back;
        }
        // where the segment's record is taken, and whether it keeps the channel's restart state for a short last segment behind it
        // (outside the fast path): iqd_wbfm.h, st_rec_plan - shared with the CPU tier's model of the hand-over
        const StRecPlan rp = st_rec_plan(q.sg.valid, q.sg.tile, q.sg.v0, q.sg.tlen, q.sg.vlen, carried_back);
        q.rec_pos = rp.park_pos;   // (= rec_pos unless the segment keeps: then its own record sits where every full segment's does, rec_pos_uniform)
        q.rec.y_in = q.cy_y;
        q.rec.y_out = q.cy_y;
        q.rec.u_out = q.cy_u;
        q.rec.back_out = rp.back_out;
        q.rec.y_end = 0.f;
        q.rec.u_end = 0.f;
        q.rec.pad[0] = q.rec.pad[1] = 0;
        const bool keeps_restart = rp.keeps_restart != 0;
        StIir s;
        s.y = 0.f; s.up = 0.f;
        s.wlast[0] = s.wlast[1] = 0;
        s.wq0[0] = s.wq0[1] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) s.y1h[k] = 0;
        s.y2lo = 0;
        s.n_sleeps = 0;
        s.ring = ring;
        s.stamps = a.stamps;
#if IQD_ST_TIMING
        s.t_wait = 0;
        s.t_seen = 0;
        s.t_to_consumed = 0;
        const long long t_iir0 = clock64();
#endif
        // (a segment that is not there has tlen 0 and stores nothing: it may run along with any kind of wave)
        // (the audio wave evaluates this very predicate: st_audio_ring_start)
        const bool fast = st_ring_is_fast(q.sg.valid, q.back, q.sg.tlen, a.tile_len, keeps_restart);
        if (keeps_restart) q.sg.valid |= 2u;
        const int rec_pos_uniform = (int)a.tile_len - FORCED_BACK;
        if (fast) {
            st_iir_lead_in(sa, rd_a, sync_a, wg, s);
            q.rec.y_in = s.y;                                    // the warmed-up state, checked against the predecessor's end
            for (int pq = ST_HALO / 32; pq < n_pieces; pq++)
                st_iir_piece<true>(a, sa, rd_a, sync_a, wg, y2r, yk, q, s, -ST_HALO + 32 * pq, lane, rec_pos_uniform);
        } else {
            for (int pq = 0; pq < n_pieces; pq++)
                st_iir_piece<false>(a, sa, rd_a, sync_a, wg, y2r, yk, q, s, -ST_HALO + 32 * pq, lane, rec_pos_uniform);
        }
        st_iir_marks(a, q, s, (int)a.tile_len, rec_pos_uniform);
        if (q.sg.valid) {
            WbfmRecord *const r = a.records + (size_t)q.sg.li * a.tiles_per_ch + q.sg.tile;
            if (q.sg.valid & 2u) {   // (the restart state this segment kept: st_iir_marks)
                q.rec.pad[0] = q.hist->pad[0];
                q.rec.pad[1] = q.hist->pad[1];
            } else if (!(q.sg.vlen - q.sg.v0 > q.sg.tlen)) {
                q.rec.pad[0] = WBFM_REC_STREAMED;   // the channel's last segment
            }
            *r = q.rec;
        }
        if (IQD_ST_WAITSTAT && lane == 0) {
            atomicAdd(&a.stamps[1], (unsigned long long)s.n_sleeps);
            atomicAdd(&a.stamps[3], (unsigned long long)n_pieces);
        }
#if IQD_ST_TIMING
        if (lane == 0) {   // per IIR wave: [28 + ring] wait, [44 + ring] total
            atomicAdd(&a.stamps[28 + ring], (unsigned long long)s.t_wait);
            atomicAdd(&a.stamps[44 + ring], (unsigned long long)(clock64() - t_iir0));
            atomicAdd(&a.stamps[60 + ring], (unsigned long long)s.t_to_consumed);
        }
#endif
    }
}

// ---- audio wave: the last decimator of every ring of the workgroup, pairs of stage-2 outputs -> PCM ---
// /2, 40 taps over the pairs p[1..20] (p[20] newest): without clamps when no loud value is in reach, else in
// the reference's order with the clamp after every MAC (Decimator_int16.cc:176-238)
template <int V>
__device__ __forceinline__ int st_audio(const StreamArgs &sa, const uint32_t (&y2p)[24], bool quiet, int c14)
{
    int acc = c14;
    if (quiet) {
        acc = dot2_from(y2p[V + 20], sa.a40p[0], c14);
#pragma unroll
        for (int q = 1; q < 20; q++) acc = dot2(y2p[V + 20 - q], ST_TAP(a40p, q), acc);
    } else {
#pragma unroll
        for (int q = 0; q < 20; q++) {
            acc = clamp_q30(dot2(y2p[V + 20 - q], ST_TAP(a40p, q) & 0xffff0000u, acc));   // newer sample of the pair: h[2q]
            acc = clamp_q30(dot2(y2p[V + 20 - q], ST_TAP(a40p, q) & 0x0000ffffu, acc));   // older: h[2q+1]
        }
    }
    return acc >> 15;
}

struct StAudRing {         // one ring's share of the audio wave: its lane's segment of that ring
    uint32_t y2p[24];      // stage-2 outputs as pairs; variant V of a piece uses [V+1 .. V+20]
    uint32_t pbuf[2];      // PCM of the first half of a 256-sample group, which leaves as one 16-byte store
    int16_t *pcm;          // the segment's first PCM sample
    uint32_t hidx;         // its boundary record, ~0u: the segment is not there
    int32_t tlen;
};

// One piece of one ring: take the pair, then the PCM sample it completes (returned).  `loud` (uniform): pieces for which a
// |y2| > AUDIO40_SAFE of ANY lane stays in reach of the 40-tap window - the ring's lanes vote, as they did inside the IIR wave.
template <int V>
__device__ __forceinline__ uint32_t st_audio_piece(const StreamArgs &sa, const StY2Ring &y2r, uint32_t &ak, StAudRing &r, int &loud, int c14)
{
    const StY2Piece yp = st_y2_piece(ak, ST_Y2_DEPTH, ST_Y2_EVERY);
    while ((int32_t)(lds_load_relaxed(y2r.full) - yp.need_full) < 0) __builtin_amdgcn_s_sleep(IQD_ST_SLEEP_A);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint32_t pair = *(const uint32_t *)(y2r.lane_slot0 + yp.slot * ST_Y2_SLOT_BYTES);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // the read has returned
    lds_signal(y2r.consumed);
    ak++;
    r.y2p[V + 20] = pair;
    const int lo = (int)(pair << 16) >> 16, hi = (int)pair >> 16;
    const uint32_t mlo = (uint32_t)(lo < 0 ? -lo : lo), mhi = (uint32_t)(hi < 0 ? -hi : hi);
    if (__any(mlo > (uint32_t)AUDIO40_SAFE || mhi > (uint32_t)AUDIO40_SAFE)) loud = 21;
    const uint32_t pcm = (uint32_t)(loud == 0 ? st_audio<V>(sa, r.y2p, true, c14) : st_audio<V>(sa, r.y2p, false, c14));
    if (loud > 0) loud--;
    return pcm;
}

// Behind a ring's four pieces at pos .. pos + 127: 128 samples = 4 PCM samples = 8 bytes.  Where the row allows it they are
// collected over 256 samples and leave as one aligned 16-byte store (segments start on multiples of 512 samples of their
// channel's stream, so the phase below is the same for every lane); else 8 bytes at a time.  (The IIR lanes collected 512
// samples for a whole 32-byte sector; three rings' worth of that - 24 registers - does not fit beside three histories.)
__device__ __forceinline__ void st_audio_quad_done(const StreamArgs &sa, StAudRing &r, int pos, bool wide, uint32_t w0, uint32_t w1)
{
    const bool valid = r.hidx != ~0u;
    if (pos >= 0 && pos < 768 - 96 && valid)   // the four pairs of this run of 128 samples, for the boundary fix-up
        ST_STORE16(&sa.hist[r.hidx].y2_first[pos >> 5], r.y2p[20], r.y2p[21], r.y2p[22], r.y2p[23]);
    if (!wide) {
        if (valid && pos >= 0 && pos < r.tlen) *(u32x2 *)(r.pcm + (pos >> 5)) = u32x2{w0, w1};
    } else if (((pos >> 7) & 1) == 0) {                  // (uniform) the group's first half waits for the second
        r.pbuf[0] = w0;
        r.pbuf[1] = w1;
    } else if (valid) {
        const int g0 = pos - 128;                        // the group [g0, g0 + 256)
        int16_t *dst = r.pcm + (g0 >> 5);
        if (g0 >= 0 && g0 + 256 <= r.tlen) {
            ST_STORE16(dst, r.pbuf[0], r.pbuf[1], w0, w1);
        } else {                                         // a segment's ragged end (or the lead-in): half by half
            if (g0 >= 0 && g0 < r.tlen) ((u32x2 *)dst)[0] = u32x2{r.pbuf[0], r.pbuf[1]};
            if (pos >= 0 && pos < r.tlen) ((u32x2 *)dst)[1] = u32x2{w0, w1};
        }
    }
#pragma unroll
    for (int k = 0; k < 20; k++) r.y2p[k] = r.y2p[k + 4];
}

// the segment's last 40 stage-2 outputs, when the quad that starts at `pos` starts behind its end (pos a multiple of 128: the
// pair history sits in y2p[0..19] here)
__device__ __forceinline__ void st_audio_end_mark(const StreamArgs &sa, const StAudRing &r, int pos)
{
    if (pos == r.tlen && r.hidx != ~0u) {
#pragma unroll
        for (int k = 0; k < 20; k += 4) ST_STORE16(&sa.hist[r.hidx].y2_last[k], r.y2p[k], r.y2p[k + 1], r.y2p[k + 2], r.y2p[k + 3]);
    }
}

// (the rings by constant index: the three rings' histories are registers only as long as nothing indexes them at run time)
static_assert(ST_RINGS == 3, "ST_FOR_RINGS names the rings");
#define ST_FOR_RINGS(...) do { { constexpr int ring = 0; __VA_ARGS__ } { constexpr int ring = 1; __VA_ARGS__ } { constexpr int ring = 2; __VA_ARGS__ } } while (0)

// What the audio wave's lane knows about its segment of ring `ring` in this round; returns the first piece the ring hands over.
__device__ __forceinline__ int st_audio_ring_start(const ChainLaunch &a, const StreamArgs &sa, uint32_t round, int ring, int lane, StAudRing &r)
{
#pragma unroll
    for (int k = 0; k < 24; k++) r.y2p[k] = 0;
    r.pbuf[0] = r.pbuf[1] = 0;
    const uint32_t sid = (round * chain_wgs(a) + chain_wg(a)) * (64u * sa.rings) + ring * 64 + lane;
    int rot_unused;
    const StSeg sg = st_segment_of(a, sa, sid, rot_unused);
    // the ring's IIR wave decides on its fast path with these very values (st_iir_wave)
    const int32_t back = sg.tile == 0 ? a.wbfm_carry[sg.ech].back : -1;
    const StRecPlan rp = st_rec_plan(sg.valid, sg.tile, sg.v0, sg.tlen, sg.vlen, sg.tile == 0 ? back : ST_HALO);
    const bool fast = st_ring_is_fast(sg.valid, back, sg.tlen, a.tile_len, rp.keeps_restart != 0);
    r.pcm = a.pcm + (size_t)sg.ch * a.pcm_stride + (sg.v0 >> 5);   // (segments start on multiples of 128 samples)
    r.hidx = sg.valid ? sg.li * a.tiles_per_ch + sg.tile : ~0u;
    r.tlen = sg.tlen;
    return fast ? ST_HALO / 32 : 0;
}

__device__ __forceinline__ void st_audio_wave(const ChainLaunch &a, const StreamArgs &sa, uint8_t *lds, uint32_t *sync, int lane)
{
    const int n_pieces = (ST_HALO + (int)a.tile_len) >> 5;       // a multiple of 4
    // wide stores need whole 512-sample groups per lane (tile_len a multiple of 512) and 32-byte aligned rows
    const bool wide = (a.tile_len & 511u) == 0 && (((uintptr_t)a.pcm | (a.pcm_stride * 2)) & 31u) == 0;
    int c14 = 1 << 14;
    asm volatile("" : "+v"(c14));
    StY2Ring y2r[ST_RINGS];
    uint32_t ak[ST_RINGS];                                       // pieces taken from each ring so far (all rounds)
    ST_FOR_RINGS(y2r[ring] = st_y2_ring(lds, sync, ring, lane); ak[ring] = 0;);
    for (uint32_t round = 0; round < sa.rounds; round++) {
        if ((round * chain_wgs(a) + chain_wg(a)) * (64u * sa.rings) >= st_id_count(sa)) break;
        StAudRing r[ST_RINGS];
        int loud[ST_RINGS], pq0[ST_RINGS];
        ST_FOR_RINGS(
            loud[ring] = 0;
            pq0[ring] = n_pieces;                                // (a ring that is not there never hands anything over)
            if (ring < (int)sa.rings) pq0[ring] = st_audio_ring_start(a, sa, round, ring, lane, r[ring]);
        );
        for (int pq = 0; pq < n_pieces; pq += 4) {
            const int pos = -ST_HALO + 32 * pq;
            // a ring's four pieces, then the next ring's: the y2 rings are deep enough for an IIR wave to go on while the
            // other two rings' quads are taken (piece by piece through the rings, the three rings' PCM words on their
            // way - six registers more - did not fit)
            ST_FOR_RINGS(if (pq >= pq0[ring]) {
                st_audio_end_mark(sa, r[ring], pos);
                const uint32_t p0 = st_audio_piece<0>(sa, y2r[ring], ak[ring], r[ring], loud[ring], c14);
                const uint32_t p1 = st_audio_piece<1>(sa, y2r[ring], ak[ring], r[ring], loud[ring], c14);
                const uint32_t p2 = st_audio_piece<2>(sa, y2r[ring], ak[ring], r[ring], loud[ring], c14);
                const uint32_t p3 = st_audio_piece<3>(sa, y2r[ring], ak[ring], r[ring], loud[ring], c14);
                st_audio_quad_done(sa, r[ring], pos, wide, pack_lo16(p0, p1), pack_lo16(p2, p3));
            });
        }
        ST_FOR_RINGS(if (ring < (int)sa.rings) st_audio_end_mark(sa, r[ring], (int)a.tile_len););
    }
}
#undef ST_FOR_RINGS

// The workgroup's whole life: table into LDS, then the waves take their roles.  (A function of its own: the kernel below
// calls it, and so does the launch that runs several families side by side, iqd_stream_mixed.hip.)
template <int ROT, bool MAG, bool EPOCHS, bool GATED>
__device__ __forceinline__ void wbfm_stream_body(const ChainLaunch &a, const StreamArgs &sa, uint8_t *st_lds)
{
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)st_lds != 0u) __builtin_trap();   // st_table_read()
    uint32_t *sync = (uint32_t *)(st_lds + ST_SYNC_OFF);
    const int tid = (int)threadIdx.x;
    {   // the table: every thread's loads in flight together, then its stores (round 5: written as one loop, the compiler waited for
        // each load before the next - nine trips to L2 one after the other at the start of every launch, 256 workgroups at once)
        constexpr int N16 = ST_TABLE_BYTES / 16, TRIPS = (N16 + ST_THREADS - 1) / ST_THREADS;
        uint4 t[TRIPS];
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const int i = tid + k * ST_THREADS;
            t[k] = ((const uint4 *)sa.half_lut)[i < N16 ? i : N16 - 1];
        }
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const int i = tid + k * ST_THREADS;
            if (i < N16) ((uint4 *)st_lds)[i] = t[k];
        }
    }
    if (tid < ST_SYNC_WORDS) sync[tid] = 0;
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    uint32_t pc = 0;                                             // pieces this wave's ring has seen (all rounds)
#if IQD_ST_TIMING   // which SIMD each of the workgroup's waves sits on (HW_ID), + 1: stamps[20000 + wave], tools/simd_of_waves.py
    if (blockIdx.x == 0 && lane == 0) a.stamps[20000 + wave] = (unsigned long long)(st_simd_id() + 1);
#endif
    if (wave < ST_RINGS) st_iir_wave(a, sa, st_lds, sync, wave, lane);
    else if (wave == ST_AUDIO_WAVE) st_audio_wave(a, sa, st_lds, sync, lane);
    else if (ROT != 2) st_p_wave<ROT, MAG, EPOCHS, GATED>(a, sa, st_lds, sync, wave - ST_RINGS, lane, pc);
    else {   // channels of several rotation selectors: the groups in their order
        st_p_wave<1, MAG, EPOCHS, GATED, true>(a, sa, st_lds, sync, wave - ST_RINGS, lane, pc);
        st_p_wave<0, MAG, EPOCHS, GATED, true>(a, sa, st_lds, sync, wave - ST_RINGS, lane, pc);
        st_p_wave<-1, MAG, EPOCHS, GATED, true>(a, sa, st_lds, sync, wave - ST_RINGS, lane, pc);
    }
}

#ifndef IQD_STREAM_BODIES_ONLY
template <int ROT, bool MAG, bool EPOCHS, bool GATED>
__global__ __launch_bounds__(ST_THREADS, 4) void wbfm_stream_kernel(const ChainLaunch a, const StreamArgs sa)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t st_lds[];
    wbfm_stream_body<ROT, MAG, EPOCHS, GATED>(a, sa, st_lds);
}
#endif

#ifndef IQD_STREAM_BODIES_ONLY
__global__ __launch_bounds__(FIX_THREADS) void wbfm_stream_fixup_kernel(const ChainLaunch a, const StreamArgs sa)
{
    __shared__ FixLds fl;
    wbfm_stream_fixup_body(a, sa, blockIdx.x, fl);
}

hipError_t launch_wbfm_stream_fixup(const ChainLaunch &a, const StreamArgs &sa, hipStream_t s)
{
    hipLaunchKernelGGL(wbfm_stream_fixup_kernel, dim3((sa.n_segments + FIX_SEGS - 1) / FIX_SEGS), dim3(FIX_THREADS), 0, s, a, sa);
    return hipGetLastError();
}

typedef void (*StKernel)(const ChainLaunch, const StreamArgs);
// [rotation selector -1, 0, +1][0: no magnitudes, 1: squelch magnitudes in the kernel, 2: squelch-gated launch][gain epochs
// within reach of a lead-in]
#define ST_K(R) {{wbfm_stream_kernel<R, false, false, false>, wbfm_stream_kernel<R, false, true, false>}, \
                 {wbfm_stream_kernel<R, true, false, false>, wbfm_stream_kernel<R, true, true, false>},   \
                 {wbfm_stream_kernel<R, false, false, true>, wbfm_stream_kernel<R, false, true, true>}}
static const StKernel st_kernels[4][3][2] = {ST_K(-1), ST_K(0), ST_K(1), ST_K(2)};   // [3]: selectors by group (StreamArgs::grouped)
#undef ST_K

// One workgroup takes nearly all of a CU's LDS; the attribute belongs to the current device's code object and is set
// once per engine by iqd_create (serialised there).
hipError_t init_wbfm_stream_kernels()
{
    for (int r = 0; r < 4; r++)
        for (int g = 0; g < 6; g++) {
            const hipError_t e = hipFuncSetAttribute((const void *)st_kernels[r][g >> 1][g & 1], hipFuncAttributeMaxDynamicSharedMemorySize, ST_LDS_BYTES);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

hipError_t launch_wbfm_stream(const ChainLaunch &a, const StreamArgs &sa, int rotation, bool mag, bool epochs, uint32_t grid, hipStream_t s)
{
    const int variant = a.vlen_gated ? 2 : (mag ? 1 : 0);
    hipLaunchKernelGGL(st_kernels[sa.grouped ? 3 : rotation < 0 ? 0 : rotation > 0 ? 2 : 1][variant][epochs ? 1 : 0], dim3(grid), dim3(ST_THREADS), ST_LDS_BYTES, s, a, sa);
    return hipGetLastError();
}

#endif   // IQD_STREAM_BODIES_ONLY

}  // namespace iqd
