// Band track measurements (include/iqdemod.h: "Band track measurements"; what the host passes: iqd_measure.h).
//
// A workgroup of four waves owns one (source, block).
//
//   row      read once: thread t takes the c = max(N / 256, 1) consecutive bins from t c (16-byte loads from c = 4 on; for
//            N < 256 the threads past N idle) and forms the excess e over the row's floor, 0 in the guard bins
//   prefix   two exclusive prefix arrays in LDS, PE[k] = sum of e below k and PK[k] = sum of k e below k, both uint64 and
//            N + 1 entries (2 x 8 x 2049 bytes at most): a thread's partial sums, an inclusive scan over the lanes of its
//            wave (shuffles), the waves' totals through LDS, then every thread writes its c entries, the last one entry N
//   slots    slot s belongs to wave s mod 4; what a slot needs is wave-uniform.  A sum over a window is a difference of two
//            prefix entries (E, sum k e, the carrier's sum).  The peak - max of e << 32 | ~k, so the lowest bin wins a tie -
//            and n_over are a strided walk of the window by the 64 lanes, e[k] = PE[k + 1] - PE[k], and a wave reduction.
//            The two OBW edges are searches on the monotone prefix in two ballots each: lane l tests the last bin of the
//            l-th stretch of ceil(span / 64) bins, the first lane that passes names the stretch, its bins are tested one per
//            lane.  Lane 0 stores the record as two 16-byte vector stores; a free or closing slot costs one load and one store
// No atomics, no second kernel, nothing to zero beforehand; the result cannot depend on the launch shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_measure.h"

namespace iqd {

__device__ __forceinline__ uint32_t msr_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ __forceinline__ uint32_t msr_first(uint64_t ballot) { return (uint32_t)__ffsll((unsigned long long)ballot) - 1; }   // ballot != 0

__global__ __launch_bounds__(MSR_WAVES * 64) void msr_kernel(const MsrLaunch a)
{
    __shared__ uint64_t s_pe[MSR_MAX_BINS + 1], s_pk[MSR_MAX_BINS + 1];
    __shared__ uint64_t s_tot[2][MSR_WAVES];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6, n = a.n;
    const size_t row = blockIdx.x;
    const uint32_t f = a.rows[row].x;
    const uint32_t c = n >= 256 ? n / 256 : 1, k0 = t * c, half = n / 2, d = a.dc_guard;
    const bool act = k0 < n;

    // the row's excess: this thread's bins k0 .. k0 + c - 1
    uint32_t ev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (act) {
        const uint32_t *p = a.power + row * n + k0;
        if (c >= 4) {
            const uint4 q0 = ((const uint4 *)p)[0];
            ev[0] = q0.x; ev[1] = q0.y; ev[2] = q0.z; ev[3] = q0.w;
            if (c == 8) {
                const uint4 q1 = ((const uint4 *)p)[1];
                ev[4] = q1.x; ev[5] = q1.y; ev[6] = q1.z; ev[7] = q1.w;
            }
        } else {
            ev[0] = p[0];
            if (c == 2) ev[1] = p[1];
        }
    }
    uint64_t se = 0, sk = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) {
        const uint32_t k = k0 + i;
        const bool guard = k + d > half && k < half + d;
        const uint32_t e = i < c && ev[i] > f && !guard ? ev[i] - f : 0;
        ev[i] = e;
        se += e;
        sk += (uint64_t)k * e;
    }

    // the prefixes: over the wave's lanes, then over the waves
    uint64_t ie = se, ik = sk;
#pragma unroll
    for (uint32_t dd = 1; dd < 64; dd <<= 1) {
        const uint64_t o1 = __shfl_up((unsigned long long)ie, dd), o2 = __shfl_up((unsigned long long)ik, dd);
        if (lane >= dd) { ie += o1; ik += o2; }
    }
    if (lane == 63) { s_tot[0][wave] = ie; s_tot[1][wave] = ik; }
    __syncthreads();
    uint64_t run_e = ie - se, run_k = ik - sk;
    for (uint32_t w = 0; w < wave; w++) { run_e += s_tot[0][w]; run_k += s_tot[1][w]; }
    if (act) {
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) {
            if (i < c) {
                s_pe[k0 + i] = run_e;
                s_pk[k0 + i] = run_k;
                run_e += ev[i];
                run_k += (uint64_t)(k0 + i) * ev[i];
            }
        }
        if (k0 + c == n) { s_pe[n] = run_e; s_pk[n] = run_k; }
    }
    __syncthreads();

    const uint32_t S = a.n_slots, m = a.margin;
    const uint4 *slots = a.slots + row * S * 2;
    uint4 *meas = a.meas + row * S * 2;
    for (uint32_t s = wave; s < S; s += MSR_WAVES) {
        const uint4 t0 = slots[2 * s], t1 = slots[2 * s + 1];
        const uint32_t id = msr_uniform(t0.x), state = msr_uniform(t0.y) & 255, bins = msr_uniform(t1.y);
        uint4 r0 = make_uint4(0, 0, 0, 0), r1 = r0;
        if (state != 0) {
            // first_bin <= last_bin < N is the tracker's promise; a table that breaks it still reads inside the row
            const uint32_t last = min(bins >> 16, n - 1), first = min(bins & 0xffff, last);
            const uint32_t lo = first > m ? first - m : 0, hi = min(last + m, n - 1);
            const uint64_t p_lo = s_pe[lo], p_hi = s_pe[hi + 1];
            const uint64_t E = p_hi - p_lo, KE = s_pk[hi + 1] - s_pk[lo];
            r0 = make_uint4(id, 0, 1u << 16, 0);                          // IQD_MEASURE_F_EMPTY
            if (E != 0) {
                // the peak (the lowest bin of the largest e) and the bins over the floor
                uint64_t key = 0;
                uint32_t over = 0;
                for (uint32_t k = lo + lane; k <= hi; k += 64) {
                    const uint32_t e = (uint32_t)(s_pe[k + 1] - s_pe[k]);
                    const uint64_t kk = (uint64_t)e << 32 | (0xffffffffu - k);
                    over += e != 0;
                    key = kk > key ? kk : key;
                }
#pragma unroll
                for (int dd = 32; dd >= 1; dd >>= 1) {
                    const uint64_t o = __shfl_xor((unsigned long long)key, dd);
                    over += (uint32_t)__shfl_xor((int)over, dd);
                    key = o > key ? o : key;
                }
                const uint32_t peak_bin = 0xffffffffu - (uint32_t)key, peak = (uint32_t)(key >> 32);

                // the occupied bandwidth: the first bin whose sum from the low end, and the last bin whose sum from the
                // high end, is more than beta E / 65536
                const uint32_t span = hi - lo + 1, stride = (span + 63) >> 6;
                const uint64_t bE = (uint64_t)a.beta * E;
                uint32_t kl = min(lo + (lane + 1) * stride - 1, hi);
                uint64_t hit = __ballot(((s_pe[kl + 1] - p_lo) << 16) > bE);            // lane 63 tests hi: L = E passes
                const uint32_t base = lo + msr_first(hit) * stride;
                kl = min(base + lane, hi);
                hit = __ballot(lane < stride && ((s_pe[kl + 1] - p_lo) << 16) > bE);
                const uint32_t obw_lo = base + msr_first(hit);
                uint32_t jl = min((lane + 1) * stride - 1, span - 1);                    // the distance below hi
                hit = __ballot(((p_hi - s_pe[hi - jl]) << 16) > bE);                     // lane 63 tests lo: R = E passes
                const uint32_t jb = msr_first(hit) * stride;
                jl = min(jb + lane, span - 1);
                hit = __ballot(lane < stride && ((p_hi - s_pe[hi - jl]) << 16) > bE);
                const uint32_t obw_hi = hi - (jb + msr_first(hit));

                const uint32_t cl = peak_bin >= lo + a.carrier_half ? peak_bin - a.carrier_half : lo;
                const uint32_t ch = min(peak_bin + a.carrier_half, hi);
                const uint32_t carrier = (uint32_t)(((s_pe[ch + 1] - s_pe[cl]) << 8) / E);
                const uint32_t centroid = (uint32_t)((KE << 8) / E);
                const bool weak = E < a.min_sum;
                const uint32_t hint = weak ? 0 : obw_hi - obw_lo + 1 >= a.wide_bins ? 3 : carrier >= a.carrier_min ? 1 : 2;
                r0 = make_uint4(id, obw_lo | obw_hi << 16, peak_bin | (weak ? 2u : 0u) << 16 | hint << 24, peak);
                r1 = make_uint4(centroid, carrier | over << 16, (uint32_t)E, (uint32_t)(E >> 32));
            }
        }
        if (lane == 0) { meas[2 * s] = r0; meas[2 * s + 1] = r1; }
    }
}

hipError_t launch_measure(const MsrLaunch &a, hipStream_t s)
{
    if (a.n_rows == 0 || a.n_rows > MSR_MAX_ROWS) return hipErrorInvalidValue;
    if (a.n < MSR_MIN_BINS || a.n > MSR_MAX_BINS || (a.n & (a.n - 1)) || a.n_slots == 0 || a.n_slots > MSR_MAX_SLOTS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(msr_kernel, dim3((uint32_t)a.n_rows), dim3(MSR_WAVES * 64), 0, s, a);
    return hipGetLastError();
}

}  // namespace iqd
