// Band activity detector (include/iqdemod.h: "Band activity"; what the host passes: iqd_detect.h).
//
// A wave owns a row of N = 64 ... 2048 uint32 powers, a workgroup DET_WAVES consecutive rows.  Everything a row needs
// crosses lanes of one wave only - ballots, shuffles and the wave's own slice of LDS - so the result cannot depend on
// the launch shape; the barriers are there for LDS ordering and every wave reaches every one of them (a wave past the
// last row redoes that row and stores nothing).
//
//   row     read once with 16-byte loads, all issued before the first is used, into the wave's LDS slice (at most 8 KiB);
//           bin 64 j + lane is lane's in word j
//   floor   exact radix select: four passes of 8 bits from the top, a 256-counter LDS histogram per pass, filled from the
//           row's pieces still in registers; lane l sums counters 4 l .. 4 l + 3, a wave prefix sum finds the lane that
//           holds the rank, it finds the digit
//   hot     the row's hot flags are ballots, one 64-bit word per 64 bins, word j kept by lane j; only words with a hot
//           bin are walked
//   words   the row's words with a hot bin are walked low to high, with the open run carried in
//           wave-uniform values: first, last, n_hot, peak key, sum, sum k p.  Inside a word, per lane:
//             previous hot bin    the highest set bit of the ballot below the lane, else the carried last hot bin
//             start               hot and (no previous hot bin or bin - previous > g + 1); a second ballot
//             sum, sum lane p     inclusive wave prefix sums (non-hot lanes add 0); a segment is a difference of two
//             peak                a segmented prefix max of (p << 32 | ~bin): the largest p, then the lowest bin
//           A start lane closes the run before it: the segment that ends at the last hot lane below it, joined with
//           the carry when no start precedes it in the word.  Closed runs pass the min_width test, a ballot and a
//           popcount give each kept one its index (runs close in ascending first_bin), and the closing lane stores the
//           record as two 16-byte vector stores.  The run still open at the row's end is closed by lane 0.
//   tail    records min(n_found, K) .. K - 1 are stored as zeros; lane 0 stores the row's 16 bytes
// No global atomics, no second kernel, nothing to zero beforehand.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_detect.h"

namespace iqd {

__device__ __forceinline__ uint32_t det_top_bit(uint64_t x) { return 63u - (uint32_t)__clzll((long long)x); }   // x != 0

__device__ __forceinline__ void det_store(uint4 *rec, uint32_t first, uint32_t last, uint32_t n_hot, uint64_t key, uint64_t sum,
                                          uint64_t ksum)
{
    const uint32_t centroid = (uint32_t)((ksum << 8) / sum);              // ksum < 2^54, sum >= 1: below 256 N
    rec[0] = make_uint4(first, last, 0xffffffffu - (uint32_t)key, (uint32_t)(key >> 32));
    rec[1] = make_uint4((uint32_t)sum, (uint32_t)(sum >> 32), centroid, n_hot);
}

constexpr int DET_PIECES = DET_MAX_BINS / 4 / 64;      // a lane's 16-byte pieces of the longest row

__global__ __launch_bounds__(DET_WAVES * 64) void det_kernel(const DetLaunch a)
{
    __shared__ uint4 s_row[DET_WAVES][DET_MAX_BINS / 4];
    __shared__ uint4 s_hist[DET_WAVES][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = a.n;
    const size_t row_raw = (size_t)blockIdx.x * DET_WAVES + wave;
    const bool live = row_raw < a.n_rows;
    const size_t row = live ? row_raw : a.n_rows - 1;

    // the row: every load is issued before the first is waited for; the pieces stay in registers for the floor
    const uint4 *src = (const uint4 *)(a.power + row * n);
    uint4 q[DET_PIECES];
#pragma unroll
    for (int j = 0; j < DET_PIECES; j++) q[j] = lane + 64 * j < n / 4 ? src[lane + 64 * j] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < DET_PIECES; j++)
        if (lane + 64 * j < n / 4) s_row[wave][lane + 64 * j] = q[j];
    __syncthreads();
    const uint32_t *p_row = (const uint32_t *)s_row[wave];
    uint32_t *hist = (uint32_t *)s_hist[wave];

    // the floor: the rank-th smallest, one byte per pass (which lane counts which bin does not matter)
    uint32_t f = 0, rank = a.rank;
#pragma unroll
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        s_hist[wave][lane] = make_uint4(0, 0, 0, 0);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < DET_PIECES; j++) {
            if (lane + 64 * j >= n / 4) continue;
            const uint32_t v4[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (pass == 0 || ((v4[c] ^ f) >> (shift + 8 & 31)) == 0) atomicAdd(&hist[(v4[c] >> shift) & 255], 1u);
        }
        __syncthreads();
        const uint4 c = s_hist[wave][lane];
        const uint32_t s = c.x + c.y + c.z + c.w;
        uint32_t incl = s;
#pragma unroll
        for (uint32_t dd = 1; dd < 64; dd <<= 1) {
            const uint32_t o = __shfl_up(incl, dd);
            if (lane >= dd) incl += o;
        }
        const uint32_t excl = incl - s;
        uint32_t r = rank - excl, dig = 4 * lane;
        if (r >= c.x) {
            r -= c.x; dig++;
            if (r >= c.y) {
                r -= c.y; dig++;
                if (r >= c.z) { r -= c.z; dig++; }
            }
        }
        const uint64_t mine = __ballot(excl <= rank && rank < incl);     // one lane: the pass counted more than rank values
        const int from = __ffsll((unsigned long long)mine) - 1;
        f |= (uint32_t)__shfl(dig, from) << shift;
        rank = __shfl(r, from);
        __syncthreads();
    }

    const uint64_t tq = ((uint64_t)(f ? f : 1u) * a.ratio_q8) >> 8;
    const uint32_t T = tq > 0xffffffffull ? 0xffffffffu : (uint32_t)tq;
    const uint32_t half = n / 2, d = a.dc_guard, g = a.bridge, m = a.min_width, K = a.max_det;
    uint4 *det = a.det + row * K * 2;

    // the hot flags: word j of the row's ballots is kept by lane j (at most 32 words)
    uint32_t h_lo = 0, h_hi = 0, hot_total = 0;
    for (uint32_t j0 = 0; j0 < n / 64; j0 += 4) {                        // four words' LDS reads in flight (N = 64, 128: the
        uint32_t pv[4];                                                   // words past the row read its last word and are cold)
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) pv[u] = p_row[min(64 * (j0 + u), n - 64) + lane];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint32_t j = j0 + u, k = 64 * j + lane;
            const uint64_t Hj = __ballot(k < n && pv[u] > T && !(k + d > half && k < half + d));
            hot_total += (uint32_t)__popcll(Hj);
            if (lane == j) { h_lo = (uint32_t)Hj; h_hi = (uint32_t)(Hj >> 32); }
        }
    }

    // the open run (wave-uniform)
    bool open = false;
    uint32_t c_first = 0, c_last = 0, c_nhot = 0;
    uint64_t c_key = 0, c_sum = 0, c_ksum = 0;
    uint32_t kept = 0;
    const uint64_t lt = (1ull << lane) - 1, le = (2ull << lane) - 1;     // the lanes below / up to this one

    for (uint64_t words = __ballot((h_lo | h_hi) != 0); words; words &= words - 1) {       // the words with a hot bin
        const uint32_t j = (uint32_t)__ffsll((unsigned long long)words) - 1, base = 64 * j;
        const uint64_t H = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)h_hi, (int)j) << 32 |
                           (uint32_t)__builtin_amdgcn_readlane((int)h_lo, (int)j);
        const uint32_t k = base + lane, p = p_row[k];
        const bool hot = (H >> lane) & 1;
        const uint64_t below = H & lt;
        const uint32_t pl = below ? det_top_bit(below) : 0;               // the last hot lane below this one
        const uint32_t prev = below ? base + pl : c_last;
        const bool start = hot && (!(below || open) || k - prev > g + 1);
        const uint64_t S = __ballot(start);

        const uint64_t v = hot ? p : 0;
        uint64_t ps = v, pk = v * lane, key = hot ? (v << 32 | (0xffffffffu - k)) : 0;
        const uint64_t sle = S & le;
        const uint32_t head = sle ? det_top_bit(sle) : 0;                 // where this lane's segment begins
#pragma unroll
        for (uint32_t dd = 1; dd < 64; dd <<= 1) {
            const uint64_t o1 = __shfl_up((unsigned long long)ps, dd), o2 = __shfl_up((unsigned long long)pk, dd);
            const uint64_t o3 = __shfl_up((unsigned long long)key, dd);
            if (lane >= dd) {
                ps += o1;
                pk += o2;
                if (lane - dd >= head && o3 > key) key = o3;
            }
        }
        const uint64_t ps_ex = ps - v, pk_ex = pk - v * lane;

        // a start lane closes the run before it: lanes h .. pl of this word, with the carry if no start precedes
        const uint64_t slt = S & lt;
        const uint32_t h = slt ? det_top_bit(slt) : 0;
        const uint64_t ps_p = __shfl((unsigned long long)ps, (int)pl), pk_p = __shfl((unsigned long long)pk, (int)pl);
        const uint64_t key_p = __shfl((unsigned long long)key, (int)pl);
        const uint64_t ps_h = __shfl((unsigned long long)ps_ex, (int)h), pk_h = __shfl((unsigned long long)pk_ex, (int)h);
        uint32_t r_first = c_first, r_last = c_last, r_nhot = c_nhot;
        uint64_t r_key = c_key, r_sum = c_sum, r_ksum = c_ksum;
        if (below) {
            r_sum = ps_p - ps_h;
            r_ksum = (uint64_t)base * r_sum + (pk_p - pk_h);
            r_nhot = (uint32_t)__popcll(H & ((2ull << pl) - 1) & ~((1ull << h) - 1));
            r_key = key_p;
            r_first = base + h;
            r_last = base + pl;
            if (!slt) {
                r_first = c_first;
                r_nhot += c_nhot;
                r_key = c_key > r_key ? c_key : r_key;
                r_sum += c_sum;
                r_ksum += c_ksum;
            }
        }
        const bool keep = start && (below || open) && r_last - r_first + 1 >= m;
        const uint64_t KM = __ballot(keep);
        const uint32_t idx = kept + (uint32_t)__popcll(KM & lt);
        if (keep && idx < K && live) det_store(det + 2 * (size_t)idx, r_first, r_last, r_nhot, r_key, r_sum, r_ksum);
        kept += (uint32_t)__popcll(KM);

        // the run open after this word
        const uint32_t q = det_top_bit(H);
        const uint64_t ps_q = __shfl((unsigned long long)ps, (int)q), pk_q = __shfl((unsigned long long)pk, (int)q);
        const uint64_t key_q = __shfl((unsigned long long)key, (int)q);
        if (S) {
            const uint32_t hs = det_top_bit(S);
            const uint64_t ps_s = __shfl((unsigned long long)ps_ex, (int)hs), pk_s = __shfl((unsigned long long)pk_ex, (int)hs);
            c_first = base + hs;
            c_nhot = (uint32_t)__popcll(H & ~((1ull << hs) - 1));
            c_key = key_q;
            c_sum = ps_q - ps_s;
            c_ksum = (uint64_t)base * c_sum + (pk_q - pk_s);
        } else {
            c_nhot += (uint32_t)__popcll(H);
            c_key = c_key > key_q ? c_key : key_q;
            c_sum += ps_q;
            c_ksum += (uint64_t)base * ps_q + pk_q;
        }
        c_last = base + q;
        open = true;
    }
    if (open && c_last - c_first + 1 >= m) {
        if (kept < K && lane == 0 && live) det_store(det + 2 * (size_t)kept, c_first, c_last, c_nhot, c_key, c_sum, c_ksum);
        kept++;
    }
    if (!live) return;
    if (lane == 0) a.rows[row] = make_uint4(f, T, kept, hot_total);
    for (uint32_t i = (kept < K ? kept : K) + lane; i < K; i += 64) {
        det[2 * (size_t)i] = make_uint4(0, 0, 0, 0);
        det[2 * (size_t)i + 1] = make_uint4(0, 0, 0, 0);
    }
}

hipError_t launch_detect(const DetLaunch &a, hipStream_t s)
{
    if (a.n_rows == 0 || a.n_rows > DET_MAX_ROWS) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((a.n_rows + DET_WAVES - 1) / DET_WAVES)), wg(DET_WAVES * 64);
    hipLaunchKernelGGL(det_kernel, grid, wg, 0, s, a);
    return hipGetLastError();
}

}  // namespace iqd
