// Band activity tracker (include/iqdemod.h: "Band tracks"; what the host passes: iqd_track.h).
//
// A wave owns a source and is a workgroup by itself, so that sources spread over CUs; lane s is slot s.  The S slots and
// next_id are read from the source's state buffer once, stay in registers over the call's blocks and go back at its end.
// Everything a block needs crosses lanes of the one wave only - readlanes, ballots, a shuffle minimum - so there is no
// LDS, no barrier, no atomic and nothing that could depend on the launch shape.
//
//   fetch     lane i holds detection i of a trip of 64 (two 16-byte loads); the next block's n_found and first trip are
//             issued before the current block is worked, further trips (K > 64 and D > 64 only) where they are needed
//   match     a wave-uniform loop over the detections: the centroid by readlane, per lane the distance to the centre as
//             the block found it, a wave minimum of dist << 6 | lane (dist < 2^19: 32 bits hold it; equal distances go to
//             the lowest lane), ~0 for a lane that is not live, already matched or out of the gate.  The winning lane
//             keeps the detection's fields.  With no winner the detection is the r-th unmatched one and the r-th lane of
//             the ballot of lanes free at the block's start keeps it (popcount rank); if there is no such lane it is
//             unplaced.
//   the rest  steps 2 .. 5 are per lane on what the loop left; a slot goes out as two 16-byte vector stores, the block's
//             record from four ballots by lane 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_track.h"

namespace iqd {

__device__ __forceinline__ uint32_t trk_wave_min(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ uint32_t trk_lane_value(uint32_t v, uint32_t j)     // j wave-uniform
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j);
}

__global__ __launch_bounds__(64) void trk_kernel(const TrkLaunch a)
{
    const uint32_t lane = threadIdx.x, src = blockIdx.x;
    const uint32_t S = a.n_slots, K = a.max_det, G = a.gate, H = a.open_hits, B = a.hold;
    const int A = (int)a.alpha;
    const uint32_t half_q8 = 128u * a.n, inc_shift = 24u - (31u - (uint32_t)__clz((int)a.n));
    const bool mine = lane < S;
    const uint64_t lt = (1ull << lane) - 1;                               // the lanes below this one
    const size_t row0 = (size_t)src * a.n_blocks;

    // the state: zeros in the lanes past S, which are never live and never free
    uint4 o0 = make_uint4(0, 0, 0, 0), o1 = o0;
    uint4 *st = a.state + ((size_t)src * S + lane) * 2;
    if (mine) { o0 = st[0]; o1 = st[1]; }
    uint32_t next_id = a.next_id[src];
    uint32_t id = o0.x, state = o0.y & 255, flags, hits = (o0.y >> 16) & 255, misses = o0.z & 0xffff, maxw = o0.z >> 16;
    uint32_t centre = o0.w, first = o1.y & 0xffff, last = o1.y >> 16, peak = o1.z, age = o1.w;

    // block 0's n_found and first trip of records
    uint32_t n_found = a.rows[row0].z;
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    if (lane < K) {
        const uint4 *p = a.det + (row0 * K + lane) * 2;
        d0 = p[0]; d1 = p[1];
    }

    for (size_t b = 0; b < a.n_blocks; b++) {
        const uint4 *det = a.det + (row0 + b) * K * 2;
        const uint32_t nf = (uint32_t)__builtin_amdgcn_readfirstlane((int)n_found), D = nf < K ? nf : K;
        uint4 c0 = d0, c1 = d1;
        if (b + 1 < a.n_blocks) {                                         // the next block's, in flight over this one's work
            n_found = a.rows[row0 + b + 1].z;
            if (lane < K) {
                const uint4 *p = det + ((size_t)K + lane) * 2;
                d0 = p[0]; d1 = p[1];
            }
        }

        // 0 clear
        if (state == 0) id = hits = misses = maxw = centre = first = last = peak = age = 0;
        flags = 0;
        const bool live0 = state != 0, free0 = mine && !live0;
        const uint32_t centre0 = centre;
        const uint32_t my_rank = (uint32_t)__popcll(__ballot(free0) & lt);

        // 1 match, and which free lane an unmatched detection goes to
        bool matched = false, taken = false;
        uint32_t mc = 0, mf = 0, ml = 0, mp = 0, unmatched = 0;
        for (uint32_t t0 = 0; t0 < D; t0 += 64) {
            if (t0 && t0 + lane < D) { c0 = det[((size_t)t0 + lane) * 2]; c1 = det[((size_t)t0 + lane) * 2 + 1]; }
            const uint32_t cnt = D - t0 < 64 ? D - t0 : 64;
            for (uint32_t j = 0; j < cnt; j++) {
                const uint32_t c = trk_lane_value(c1.z, j), f = trk_lane_value(c0.x, j), l = trk_lane_value(c0.y, j);
                const uint32_t p = trk_lane_value(c0.w, j);
                const uint32_t dist = centre0 > c ? centre0 - c : c - centre0;
                const uint32_t key = live0 && !matched && dist <= G ? (dist << 6 | lane) : 0xffffffffu;
                const uint32_t m = trk_wave_min(key);
                const bool none = m == 0xffffffffu;
                const bool win = none ? free0 && my_rank == unmatched : lane == (m & 63);
                if (win) { mc = c; mf = f; ml = l; mp = p; }
                matched |= win && !none;
                taken |= win && none;
                unmatched += none;
            }
        }
        const uint32_t n_free = (uint32_t)__popcll(__ballot(free0));
        const uint32_t placed = unmatched < n_free ? unmatched : n_free;

        // 2 update
        if (matched) {
            centre = (uint32_t)((int)centre + ((((int)mc - (int)centre) * A) >> 8));
            first = mf; last = ml; peak = mp;
            const uint32_t w = ml - mf + 1;
            maxw = w > maxw ? w : maxw;
            hits = hits < 255 ? hits + 1 : 255;
            misses = 0;
            flags |= 1;
            if (state == 1 && hits >= H) { state = 2; flags |= 4; }
        }
        // 3 age
        if (live0) {
            age++;
            if (!matched) {
                misses++;
                if (state == 1) id = state = hits = misses = maxw = centre = first = last = peak = age = 0;
                else if (misses > B) { state = 0; flags |= 8; }
            }
        }
        // 4 allocate
        if (taken) {
            id = next_id + my_rank + 1;
            state = H == 1 ? 2 : 1;
            flags = H == 1 ? 7 : 3;
            hits = 1; misses = 0; centre = mc; age = 0;
            first = mf; last = ml; peak = mp; maxw = ml - mf + 1;
        }
        next_id += placed;
        // 5 derive
        uint32_t phase = 0, cls = 0;
        if (id != 0) {
            phase = ((centre - half_q8) << inc_shift) + a.inc_bias;
            cls = (maxw >= a.edge0) + (maxw >= a.edge1) + (maxw >= a.edge2);
        }

        o0 = make_uint4(id, state | flags << 8 | hits << 16 | cls << 24, (misses & 0xffff) | maxw << 16, centre);
        o1 = make_uint4(phase, first | last << 16, peak, age);
        if (mine) {
            uint4 *out = a.slots + ((row0 + b) * S + lane) * 2;
            out[0] = o0; out[1] = o1;
        }
        const uint32_t n_act = (uint32_t)__popcll(__ballot(state == 2)), n_ten = (uint32_t)__popcll(__ballot(state == 1));
        const uint32_t n_op = (uint32_t)__popcll(__ballot((flags & 4) != 0)), n_cl = (uint32_t)__popcll(__ballot((flags & 8) != 0));
        if (lane == 0) a.blocks[row0 + b] = make_uint4(n_act, n_ten, n_op | n_cl << 16, unmatched - placed);
    }

    if (mine) { st[0] = o0; st[1] = o1; }
    if (lane == 0) a.next_id[src] = next_id;
}

hipError_t launch_track(const TrkLaunch &a, hipStream_t s)
{
    if (a.n_sources == 0 || a.n_blocks == 0 || a.n_blocks > TRK_MAX_ROWS / a.n_sources) return hipErrorInvalidValue;
    if (a.n_slots == 0 || a.n_slots > TRK_MAX_SLOTS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(trk_kernel, dim3(a.n_sources), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace iqd
