// WBFM streaming pipeline: what a lane knows about its segment, and the boundary fix-up that follows the stream kernel
// (iqd_stream.hip).  A header because the fix-up also runs as one role of the launch that finishes several families'
// streaming kernels at once (iqd_kernels.hip: mixed_tail_kernel).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "iqd_kernels.h"
#include "iqd_stream.h"
#include "iqd_stream_mixed.h"
#include "iqd_wbfm.h"
#include "iqd_mfma.h"

namespace iqd {

struct StSeg {           // what a lane knows about its segment
    uint32_t valid, li, tile, ch, ech;
    int32_t v0, tlen;
    int32_t vlen;        // samples the channel consumes in this call: all of them, or those of its open blocks (squelch-gated call)
};

__device__ __forceinline__ StSeg st_segment(const ChainLaunch &a, uint32_t sid, uint32_t n_segments)
{
    StSeg s;
    s.valid = sid < n_segments ? 1u : 0u;
    const uint32_t id = s.valid ? sid : 0u;
    s.li = id / a.tiles_per_ch;
    s.tile = id - s.li * a.tiles_per_ch;
    s.ch = a.ch_list[s.li];
    s.ech = a.first_ch + s.ch;
    // a squelch-gated call: the chain sees the concatenation of the channel's open blocks (IqDataProcessor.cc:793), a
    // virtual stream of vlen_gated[ch] samples, and the segments are cut on that axis
    const uint32_t vlen = a.vlen_gated ? a.vlen_gated[s.ch] : a.vlen;
    s.vlen = (int32_t)vlen;
    const int64_t v0 = (int64_t)s.tile * a.tile_len;
    if (v0 >= (int64_t)vlen) { s.valid = 0; s.v0 = 0; s.tlen = 0; return s; }
    s.v0 = (int32_t)v0;
    const int64_t rest = (int64_t)vlen - v0;
    s.tlen = (int32_t)(rest < (int64_t)a.tile_len ? rest : (int64_t)a.tile_len);
    if (!s.valid) s.tlen = 0;
    return s;
}

// The same for a launch whose ids are grouped by rotation selector (StreamArgs::grouped); rot = the id's selector.
// (IQD_ST_NO_GROUPS: a translation unit whose launches are never grouped - the one that holds all four families' pipelines,
// iqd_stream_mixed.hip, where every scalar register counts - compiles the plain mapping only.)
#ifndef IQD_ST_NO_GROUPS
#define IQD_ST_NO_GROUPS 0
#endif
__device__ __forceinline__ StSeg st_segment_of(const ChainLaunch &a, const StreamArgs &sa, uint32_t sid, int &rot)
{
    if (IQD_ST_NO_GROUPS || !sa.grouped) { rot = 0; return st_segment(a, sid, sa.n_segments); }
    const uint32_t r = (sid >= sa.group_start[1] ? 1u : 0u) + (sid >= sa.group_start[2] ? 1u : 0u);
    rot = 1 - (int)r;
    const uint32_t local = sid - sa.group_start[r];
    const bool there = sid < sa.group_start[3] && local < sa.group_nseg[r];
    // (an id that is padding maps to no segment: st_segment() then hands back the launch's first channel with length 0)
    return st_segment(a, there ? sa.group_li0[r] * a.tiles_per_ch + local : sa.n_segments, sa.n_segments);
}
__device__ __forceinline__ uint32_t st_id_count(const StreamArgs &sa) { return !IQD_ST_NO_GROUPS && sa.grouped ? sa.group_start[3] : sa.n_segments; }

// The first ST_FIX_PCM PCM samples of every cold segment, recomputed with the exact histories its predecessor left
// (StHist): stage-1 output 0, stage-2 outputs 0..2, then the 40-tap audio decimator in the reference's MAC order with
// the clamp after every MAC (Decimator_int16.cc:176-238) - or, where no |y2| in the boundary's reach exceeds AUDIO40_SAFE, the
// clamp-free sum, which equals it when no clamp can fire (the audio wave's rule: st_audio).  A workgroup takes FIX_SEGS consecutive
// segments: their FIX_SEGS + 1 records (the predecessor of the first included) are one contiguous read into LDS (16 + 1 records:
// 4352 bytes, a 16-byte load per thread and a second one for 16 threads); then FIX_LANES threads per segment, a PCM sample (or two) each.
// (round 6: IQD_FIX_LANES threads per segment - 32 in rounds 2-5, one per PCM sample with 11 idle; 16 with two samples for the first
// five halve the launch's waves, and its workgroups then nearly fit the chip at once: the kernel is its trips to memory)
#ifndef IQD_FIX_LANES
#define IQD_FIX_LANES 16
#endif
constexpr int FIX_LANES = IQD_FIX_LANES;
constexpr int FIX_SEGS = 256 / FIX_LANES;
constexpr int FIX_THREADS = FIX_LANES * FIX_SEGS;
static_assert(FIX_LANES == 16 || FIX_LANES == 32, "threads per boundary");
struct FixLds {
    alignas(16) uint32_t rec[(FIX_SEGS + 1) * 64];   // (staged with 16-byte stores)
    uint32_t y2x[FIX_SEGS][41];             // per segment: stage-2 pairs -40 .. 41 with the boundary ones exact
};
static_assert(sizeof(FixLds) == ((FIX_SEGS + 1) * 64 + FIX_SEGS * 41) * 4, "the alignment adds no padding (a union member of mixed_tail_kernel's LDS)");
__device__ __forceinline__ void wbfm_stream_fixup_body(const ChainLaunch &a, const StreamArgs &sa, const uint32_t block, FixLds &fl)
{
    uint32_t (&rec)[(FIX_SEGS + 1) * 64] = fl.rec;
    uint32_t (&y2x)[FIX_SEGS][41] = fl.y2x;
    const uint32_t sid0 = block * FIX_SEGS;
    const int tid = (int)threadIdx.x, sl = tid / FIX_LANES, i = tid % FIX_LANES;
    // Everything this workgroup needs from memory is asked for at once and waited for once, in front of the first barrier:
    // the FIX_SEGS + 1 records as 16-byte loads (one per thread and a second one for the first 16 threads: the index is
    // clamped, not branched around, as the stream kernel copies its table), the two states of the hand-off, whose addresses
    // take the segment's id only, and the segment's channel - which nothing needs before the PCM address in a launch
    // that is not squelch-gated; a gated one goes for its channel's length with it, one dependent trip.  (Round 2 made it
    // "at once" in the source: 17.6 us of latency for 47 662 boundaries.  The compiled kernel still waited for the channel
    // first, then ran the staging as a loop of single dwords with a wait in each of its five turns: six trips one after the other.)
    const uint32_t sid = sid0 + (uint32_t)sl;
    const bool there = sid < sa.n_segments;
    StSeg sg;                                          // st_segment() of the id, with the channel asked for last
    sg.li = (there ? sid : 0u) / a.tiles_per_ch;
    sg.tile = (there ? sid : 0u) - sg.li * a.tiles_per_ch;
    constexpr int REC16 = (FIX_SEGS + 1) * 16, TRIPS = (REC16 + FIX_THREADS - 1) / FIX_THREADS;
    const uint32_t n_avail = (sa.n_segments - sid0 < (uint32_t)FIX_SEGS ? sa.n_segments - sid0 : (uint32_t)FIX_SEGS) + (sid0 ? 1u : 0u);
    const uint32_t n16 = n_avail * 16;                 // (the launch's first workgroup has no predecessor record, its last one fewer segments)
    v4u t[TRIPS];
    {
        const v4u *src = (const v4u *)sa.hist + ((size_t)sid0 - (sid0 ? 1 : 0)) * 16;
#pragma unroll
        for (int k = 0; k < TRIPS; k++) {
            const uint32_t k16 = (uint32_t)(tid + k * FIX_THREADS);
            t[k] = src[k16 < n16 ? k16 : n16 - 1];
        }
    }
    float y_in = 0.f, y_end = 0.f;
    if (i == FIX_LANES - 1) {                          // (a segment that is not live: some record of the launch, not looked at)
        const WbfmRecord *r = a.records + (size_t)sg.li * a.tiles_per_ch;
        y_in = r[sg.tile].y_in;
        y_end = r[sg.tile ? sg.tile - 1 : 0].y_end;
    }
    sg.ch = a.ch_list[sg.li];
    sg.ech = a.first_ch + sg.ch;
    sg.vlen = (int32_t)(a.vlen_gated ? a.vlen_gated[sg.ch] : a.vlen);
    {
        const int64_t v0 = (int64_t)sg.tile * a.tile_len, rest = (int64_t)(uint32_t)sg.vlen - v0;
        sg.valid = there && rest > 0 ? 1u : 0u;
        sg.v0 = sg.valid ? (int32_t)v0 : 0;
        sg.tlen = !sg.valid ? 0 : (int32_t)(rest < (int64_t)a.tile_len ? rest : (int64_t)a.tile_len);
    }
    const bool live = sg.valid && sg.tile != 0;
    // (the loads stay where they are: left alone, the compiler moves each into the branch of its store, with a wait of its own)
    static_assert(TRIPS == 1 || TRIPS == 2, "one statement names all of a thread's loads: one wait");
    if constexpr (TRIPS == 2) asm volatile("" : "+v"(t[0]), "+v"(t[TRIPS - 1]));
    else asm volatile("" : "+v"(t[0]));
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
        const uint32_t k16 = (uint32_t)(tid + k * FIX_THREADS);
        if (k16 < n16) ((v4u *)rec)[k16 + (sid0 ? 0 : 16)] = t[k];
    }
    __syncthreads();
    const StHist &prev = *(const StHist *)&rec[sl * 64], &own = *(const StHist *)&rec[(sl + 1) * 64];
    if (live && i < 3) {                               // stage-2 output i (0..2) of the segment, from y1[4i-8 .. 4i+3]
        int acc = 1 << 14;                             // stage-1 output 0: w[-4 .. 3]
        acc = dot2(prev.w_last[0], sa.d1p[0], acc);
        acc = dot2(prev.w_last[1], sa.d1p[1], acc);
        acc = dot2(own.w_first[0], sa.d1p[2], acc);
        acc = dot2(own.w_first[1], sa.d1p[3], acc);
        uint32_t y1[10];                               // pairs: outputs -8 .. 11
#pragma unroll
        for (int k = 0; k < 4; k++) y1[k] = prev.y1_last[k];
#pragma unroll
        for (int k = 0; k < 6; k++) y1[4 + k] = own.y1_first[k];
        y1[4] = (y1[4] & 0xffff0000u) | ((uint32_t)(acc >> 15) & 0xffffu);
        int s2 = 1 << 14;
#pragma unroll
        for (int q = 0; q < 6; q++) {
            const uint32_t d = i == 0 ? y1[5 - q] : (i == 1 ? y1[7 - q] : y1[9 - q]);   // pairs 2i .. 2i+5, newest first
            s2 = dot2(d, sa.p12p[q], s2);
        }
        ((int16_t *)&y2x[sl][20])[i] = (int16_t)(s2 >> 15);   // outputs 0, 1 -> pair 20; output 2 -> low half of pair 21
    } else if (live) {                                 // the other pairs as they are (each thread a few)
        for (int p = i - 3; p < 41; p += FIX_LANES - 3) {
            if (p == 20) continue;
            if (p == 21) ((int16_t *)&y2x[sl][21])[1] = (int16_t)(own.y2_first[1] >> 16);
            else y2x[sl][p] = p < 20 ? prev.y2_last[p] : own.y2_first[p - 20];
        }
    }
    // Hand-off verification of the same segments (what wbfm_verify_kernel does for tile launches): a cold segment's
    // warmed-up state at its start must be its predecessor's end state, bit for bit.  Only mismatches touch the
    // device counters (thousands of workgroups adding to one word would cost more than the whole kernel); the host
    // knows how many hand-offs a launch has.
    if (live && i == FIX_LANES - 1 && f2u(y_in) != f2u(y_end)) {   // (bit-equal is the rule; the sub-2^-100 exception needs the channel's K: rare)
        if (!iir_states_agree(y_in, y_end, a.params[sg.ech].wbfm_k >= 1.0f)) {
            atomicAdd(&a.counters[CNT_TILE_MISMATCH], 1u);
            atomicAdd(&a.counters[CNT_STREAM_MISMATCH], 1u);
            a.repair_flags[sg.li] = 1;
        }
    }
    __syncthreads();   // y2x[sl] was written by this segment's 32 threads, each reads the others' entries (uniform control flow up to here)
    if (!live) return;
    // Once per boundary: does any of its pairs hold a |y2| that can make the 40-tap sum clamp?  If none does, the sum without
    // clamps is what the reference's clamped one gives (st_audio of the stream kernel, wbfm_stage3 of the tile kernels) -
    // 20 dependent v_dot2 instead of 40 with a clamp behind each.  A boundary's FIX_LANES lanes vote; they sit in one wave.
    bool loud_lane = false;
    for (int p = i; p < 41; p += FIX_LANES) {
        const uint32_t pair = y2x[sl][p];
        const int lo = (int)(pair << 16) >> 16, hi = (int)pair >> 16;
        loud_lane |= (uint32_t)(lo < 0 ? -lo : lo) > (uint32_t)AUDIO40_SAFE || (uint32_t)(hi < 0 ? -hi : hi) > (uint32_t)AUDIO40_SAFE;
    }
    const uint64_t lanes_of_boundary = (FIX_LANES == 32 ? 0xffffffffull : 0xffffull) << ((tid & 63) / FIX_LANES * FIX_LANES);
    const bool quiet = (__ballot(loud_lane) & lanes_of_boundary) == 0;
    int16_t *pcm = a.pcm + (size_t)sg.ch * a.pcm_stride + (sg.v0 >> 5);
    if (quiet) {
        for (int j = i; j < ST_FIX_PCM && j < sg.tlen / 32; j += FIX_LANES) {
            // PCM j from stage-2 outputs 2j-38 .. 2j+1: pairs j+1 .. j+20, newest first
            int s3 = 1 << 14;
#pragma unroll
            for (int q = 0; q < 20; q++) s3 = dot2(y2x[sl][20 + j - q], sa.a40p[q], s3);
            pcm[j] = (int16_t)(s3 >> 15);
        }
    } else {
        uint32_t newer[20], older[20];                 // the taps of a pair one at a time: on the scalar side, once
#pragma unroll
        for (int q = 0; q < 20; q++) {
            newer[q] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(sa.a40p[q] & 0xffff0000u));   // h[2q]
            older[q] = (uint32_t)__builtin_amdgcn_readfirstlane((int)(sa.a40p[q] & 0x0000ffffu));   // h[2q+1]
        }
        for (int j = i; j < ST_FIX_PCM && j < sg.tlen / 32; j += FIX_LANES) {
            int s3 = 1 << 14;                          // the reference's order, the clamp after every MAC
#pragma unroll
            for (int q = 0; q < 20; q++) {
                const uint32_t pair = y2x[sl][20 + j - q];
                s3 = clamp_q30(dot2(pair, newer[q], s3));
                s3 = clamp_q30(dot2(pair, older[q], s3));
            }
            pcm[j] = (int16_t)(s3 >> 15);
        }
    }
}

}  // namespace iqd
