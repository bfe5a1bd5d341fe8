// Band track log (include/iqdemod.h: "Band track log"; what the host passes: iqd_tracklog.h).
//
// The tracker's shape: a wave owns a source and is a workgroup by itself, so that sources spread over CUs; lane s is slot s.
// The S summaries and the source's block index g are read from the state buffer once, stay in registers over the call's
// blocks and go back at its end.  What crosses lanes is two ballots' popcounts per block, so there is no LDS, no barrier, no
// atomic and nothing that could depend on the launch shape.
//
//   fetch     a lane reads the first 16 bytes of its slot (track_id, state, width_class and centre_q8 all lie there) and the
//             32 bytes of its measurement record; the next block's three loads are issued before the current block is worked
//   a block   steps 0 .. 4 of the header per lane on registers; the summary goes out as four 16-byte vector stores
//   events    a lane ends at most one track that is an event per block (a track that starts and closes in one block has no
//             active block).  Its place is the wave-uniform count of the call's events so far plus the popcount of the
//             block's ballot below the lane - block order, then slot order; a place >= E stores nothing
//   the end   the state goes back, the lanes zero events[n_stored .. E) - behind the event stores of the same wave in program
//             order, and on other addresses anyway - and lane 0 stores the counts
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_tracklog.h"

namespace iqd {

constexpr uint32_t TLG_F_NEW = 1, TLG_F_MODE_CHANGED = 2, TLG_F_CLOSED = 4, TLG_F_LOST = 8;

// a summary in registers; pack() is the record's four quarters
struct TlgSummary {
    uint32_t id, state, mode, cls, n_blocks, n_active, n_measured, v0, v1, v2, peak, lo, hi;
    uint64_t first_block, sum_centre, sum_excess;
};

__device__ __forceinline__ void tlg_unpack(TlgSummary &s, const uint4 &q0, const uint4 &q1, const uint4 &q2, const uint4 &q3)
{
    s.id = q0.x; s.state = q0.y & 255; s.mode = (q0.y >> 16) & 255; s.cls = q0.y >> 24;
    s.first_block = (uint64_t)q0.w << 32 | q0.z;
    s.n_blocks = q1.x; s.n_active = q1.y; s.n_measured = q1.z; s.v0 = q1.w;
    s.v1 = q2.x; s.v2 = q2.y; s.sum_centre = (uint64_t)q2.w << 32 | q2.z;
    s.sum_excess = (uint64_t)q3.y << 32 | q3.x; s.peak = q3.z; s.lo = q3.w & 0xffff; s.hi = q3.w >> 16;
}

__device__ __forceinline__ void tlg_pack(const TlgSummary &s, uint32_t flags, uint4 &q0, uint4 &q1, uint4 &q2, uint4 &q3)
{
    q0 = make_uint4(s.id, s.state | flags << 8 | s.mode << 16 | s.cls << 24, (uint32_t)s.first_block, (uint32_t)(s.first_block >> 32));
    q1 = make_uint4(s.n_blocks, s.n_active, s.n_measured, s.v0);
    q2 = make_uint4(s.v1, s.v2, (uint32_t)s.sum_centre, (uint32_t)(s.sum_centre >> 32));
    q3 = make_uint4((uint32_t)s.sum_excess, (uint32_t)(s.sum_excess >> 32), s.peak, s.lo | s.hi << 16);
}

__device__ __forceinline__ void tlg_clear(TlgSummary &s)
{
    s.id = s.state = s.mode = s.cls = s.n_blocks = s.n_active = s.n_measured = s.v0 = s.v1 = s.v2 = s.peak = s.lo = s.hi = 0;
    s.first_block = s.sum_centre = s.sum_excess = 0;
}

__device__ __forceinline__ uint4 tlg_select(bool p, const uint4 &x, const uint4 &y)     // by value, word by word: registers only
{
    return make_uint4(p ? x.x : y.x, p ? x.y : y.y, p ? x.z : y.z, p ? x.w : y.w);
}

__device__ __forceinline__ uint32_t tlg_count(bool p) { return (uint32_t)__popcll(__ballot(p)); }

__global__ __launch_bounds__(64) void tlg_kernel(const TlgLaunch a)
{
    const uint32_t lane = threadIdx.x, src = blockIdx.x;
    const uint32_t S = a.n_slots, E = a.max_events, A = a.min_active, VM = a.vote_min;
    const bool mine = lane < S;
    const uint64_t lt = (1ull << lane) - 1;                               // the lanes below this one
    const size_t row0 = (size_t)src * a.n_blocks;
    const uint4 zero = make_uint4(0, 0, 0, 0);

    // the state: zeros in the lanes past S, which see free slots only and so never hold a track
    uint4 o0 = zero, o1 = zero, o2 = zero, o3 = zero;
    uint4 *st = a.state + ((size_t)src * S + lane) * 4;
    if (mine) { o0 = st[0]; o1 = st[1]; o2 = st[2]; o3 = st[3]; }
    uint64_t g = a.g[src];
    TlgSummary s;
    tlg_unpack(s, o0, o1, o2, o3);
    uint32_t flags = (o0.y >> 8) & 255;                                   // what get_state shows; every block clears it first

    uint4 *ev = a.events + (size_t)src * E * 4;
    uint32_t n_events = 0, n_short = 0, n_lost = 0;                       // wave-uniform

    // block 0's slot and record
    uint4 nt = zero, nm0 = zero, nm1 = zero;
    if (mine) {
        nt = a.slots[(row0 * S + lane) * 2];
        const uint4 *p = a.meas + (row0 * S + lane) * 2;
        nm0 = p[0]; nm1 = p[1];
    }

    for (size_t b = 0; b < a.n_blocks; b++) {
        const uint4 t = nt, m0 = nm0, m1 = nm1;
        if (mine && b + 1 < a.n_blocks) {                                 // the next block's, in flight over this one's work
            const size_t i = ((row0 + b + 1) * S + lane) * 2;
            nt = a.slots[i];
            nm0 = a.meas[i]; nm1 = a.meas[i + 1];
        }
        const uint32_t tid = t.x, tstate = t.y & 255;
        flags = 0;

        // 0 vanished: the record as it stood, flag lost, is the event
        const bool lost = s.id != 0 && tid != s.id;
        const bool lost_event = lost && s.n_active >= A;
        uint4 e0 = zero, e1 = zero, e2 = zero, e3 = zero;
        if (lost) {
            tlg_pack(s, TLG_F_LOST, e0, e1, e2, e3);
            tlg_clear(s);
        }
        // 1 start.  From here on s.id == tid: a table slot without an id is free whatever its state says
        if (tid != 0 && s.id == 0) {
            s.id = tid; s.first_block = g; s.lo = 0xffff;
            flags = TLG_F_NEW;
        }
        bool closed = false, closed_event = false;
        if (s.id != 0) {
            // 2 accumulate
            if (tstate != 0) {
                s.n_blocks++;
                s.state = tstate; s.cls = t.y >> 24;
                if (tstate == 2) { s.n_active++; s.sum_centre += t.w; }
                const uint32_t mflags = (m0.z >> 16) & 255, hint = m0.z >> 24;
                if (m0.x == tid && mflags == 0) {
                    const uint32_t lo = m0.y & 0xffff, hi = m0.y >> 16;
                    s.n_measured++;
                    s.sum_excess += (uint64_t)m1.w << 32 | m1.z;
                    s.peak = m0.w > s.peak ? m0.w : s.peak;
                    s.lo = lo < s.lo ? lo : s.lo;
                    s.hi = hi > s.hi ? hi : s.hi;
                    s.v0 += hint == 1; s.v1 += hint == 2; s.v2 += hint == 3;
                }
            }
            // 3 decide: the most votes, a tie to the lowest hint
            uint32_t mode = 0;
            if (s.v0 + s.v1 + s.v2 >= VM) {
                uint32_t best = s.v0;
                mode = 1;
                if (s.v1 > best) { best = s.v1; mode = 2; }
                if (s.v2 > best) mode = 3;
            }
            if (mode != s.mode) flags |= TLG_F_MODE_CHANGED;
            s.mode = mode;
            // 4 close
            if (tstate == 0) {
                closed = true;
                closed_event = s.n_active >= A;
                flags |= TLG_F_CLOSED;
                s.state = 0;
            }
        }
        tlg_pack(s, flags, o0, o1, o2, o3);                               // a free slot: s is all zero, and so are the flags
        if (mine) {
            uint4 *out = a.summary + ((row0 + b) * S + lane) * 4;
            out[0] = o0; out[1] = o1; out[2] = o2; out[3] = o3;
        }

        // the block's events, in slot order behind the call's earlier ones
        const bool emit = lost_event || closed_event;                     // never both: see the head of the file
        const uint64_t em = __ballot(emit);
        if (em != 0) {
            const uint32_t place = n_events + (uint32_t)__popcll(em & lt);
            if (emit && place < E) {
                uint4 *out = ev + (size_t)place * 4;
                out[0] = tlg_select(lost_event, e0, o0); out[1] = tlg_select(lost_event, e1, o1);
                out[2] = tlg_select(lost_event, e2, o2); out[3] = tlg_select(lost_event, e3, o3);
            }
            n_events += (uint32_t)__popcll(em);
            n_lost += tlg_count(lost_event);
        }
        n_short += tlg_count(lost && !lost_event) + tlg_count(closed && !closed_event);
        if (closed) {
            tlg_clear(s);
            flags = 0;
            o0 = o1 = o2 = o3 = zero;
        }
        g++;
    }

    if (mine) { st[0] = o0; st[1] = o1; st[2] = o2; st[3] = o3; }
    if (lane == 0) a.g[src] = g;
    const uint32_t n_stored = n_events < E ? n_events : E;
    for (uint32_t i = n_stored + lane; i < E; i += 64) {
        uint4 *out = ev + (size_t)i * 4;
        out[0] = zero; out[1] = zero; out[2] = zero; out[3] = zero;
    }
    if (lane == 0) a.counts[src] = make_uint4(n_events, n_stored, n_short, n_lost);
}

hipError_t launch_tracklog(const TlgLaunch &a, hipStream_t s)
{
    if (a.n_sources == 0 || a.n_blocks == 0 || a.n_blocks > TLG_MAX_ROWS / a.n_sources) return hipErrorInvalidValue;
    if (a.n_slots == 0 || a.n_slots > TLG_MAX_SLOTS || a.max_events == 0 || a.max_events > TLG_MAX_EVENTS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tlg_kernel, dim3(a.n_sources), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace iqd
