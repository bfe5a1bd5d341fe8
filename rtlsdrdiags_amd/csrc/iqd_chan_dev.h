// Device pieces of the wideband channelizer shared by chz_kernel / chz_scan_kernel (iqd_chan.hip), the fractional-rate
// chz_frac_kernel (iqd_chan_frac.hip) and chz_survey_kernel (iqd_chan_survey.hip): the B operand read, the epilogue of one
// output, the window staging.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan.h"

namespace iqd {

typedef int chz_v4i __attribute__((ext_vector_type(4)));
typedef short chz_s2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int32_t chz_sat(int32_t x, int32_t lo, int32_t hi) { return min(max(x, lo), hi); }

__device__ __forceinline__ void chz_wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// B operand: 16 window bytes at LDS byte offset o (o even)
__device__ __forceinline__ chz_v4i chz_b_operand(const uint8_t *win, uint32_t o)
{
    const uint32_t *w = (const uint32_t *)(win + (o & ~3u));
    const uint32_t sh = o & 3u;
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
    chz_v4i b;
    b.x = (int)__builtin_amdgcn_alignbyte(w1, w0, sh);
    b.y = (int)__builtin_amdgcn_alignbyte(w2, w1, sh);
    b.z = (int)__builtin_amdgcn_alignbyte(w3, w2, sh);
    b.w = (int)__builtin_amdgcn_alignbyte(w4, w3, sh);
    return b;
}

// one channel's output at one sample: the two rails' accumulators (lo / hi planes) -> two offset-binary bytes
__device__ __forceinline__ uint32_t chz_epilogue(int32_t rlo, int32_t rhi, int32_t ilo, int32_t ihi, uint32_t p,
                                                 int32_t rnd, uint32_t sh)
{
    // A = lo + 256 hi + 128 fits int32 (the tap bounds), but 256 hi alone need not: combined modulo 2^32
    const int32_t Ar = (int32_t)((uint32_t)rlo + ((uint32_t)rhi << 8) + 128u);
    const int32_t Ai = (int32_t)((uint32_t)ilo + ((uint32_t)ihi << 8) + 128u);
    const int32_t ar = chz_sat(Ar >> 8, -32768, 32767);
    const int32_t ai = chz_sat(Ai >> 8, -32768, 32767);
    const int32_t c = (int16_t)(p & 0xffffu), s = (int16_t)(p >> 16);
    const chz_s2 va = {(short)ar, (short)ai};
    const chz_s2 vb = {(short)ai, (short)ar};
    const chz_s2 cs = {(short)c, (short)s};
    const chz_s2 cns = {(short)c, (short)-s};                          // |s| <= 32767: -s fits
    const int32_t rr = __builtin_amdgcn_sdot2(va, cs, 0, false);       // ar c + ai s
    const int32_t ri = __builtin_amdgcn_sdot2(vb, cns, 0, false);      // ai c - ar s
    const int32_t yr = chz_sat((rr + rnd) >> sh, -128, 127), yi = chz_sat((ri + rnd) >> sh, -128, 127);
    return (uint32_t)(yr + 128) | ((uint32_t)(yi + 128) << 8);
}

// chz_epilogue up to the rotation (chz_gain_kernel, iqd_chan_gain.hip): stage a and rr = ar c + ai s, ri = ai c - ar s,
// |rr|, |ri| < 2^31
__device__ __forceinline__ void chz_epilogue_rot(int32_t rlo, int32_t rhi, int32_t ilo, int32_t ihi, uint32_t p, int32_t &rr,
                                                 int32_t &ri)
{
    const int32_t Ar = (int32_t)((uint32_t)rlo + ((uint32_t)rhi << 8) + 128u);
    const int32_t Ai = (int32_t)((uint32_t)ilo + ((uint32_t)ihi << 8) + 128u);
    const int32_t ar = chz_sat(Ar >> 8, -32768, 32767);
    const int32_t ai = chz_sat(Ai >> 8, -32768, 32767);
    const int32_t c = (int16_t)(p & 0xffffu), s = (int16_t)(p >> 16);
    const chz_s2 va = {(short)ar, (short)ai};
    const chz_s2 vb = {(short)ai, (short)ar};
    const chz_s2 cs = {(short)c, (short)s};
    const chz_s2 cns = {(short)c, (short)-s};
    rr = __builtin_amdgcn_sdot2(va, cs, 0, false);
    ri = __builtin_amdgcn_sdot2(vb, cns, 0, false);
}

// The gain in dB as the last step (include/iqdemod.h: "Gain-following channels"): g = 6 e + j, m_j = lrint(4096 2^(j/6)).
// Mantissa and exponent of one gain as one word, (m_j << 4) | e; g <= 48, so e <= 8.
__host__ __device__ __forceinline__ uint32_t chz_gain_split(uint32_t g)
{
    const uint32_t e = g / 6, j = g - 6 * e;
    const uint32_t m = j == 0 ? IQD_GAIN_M0 : j == 1 ? IQD_GAIN_M1 : j == 2 ? IQD_GAIN_M2 : j == 3 ? IQD_GAIN_M3
                     : j == 4 ? IQD_GAIN_M4 : IQD_GAIN_M5;
    return (m << 4) | e;
}
// One rail: t = floor(r m_j / 2^14) as the high word of r (m_j 2^18) (m_j 2^18 < 2^31, |t| < 2^30), then
// y = sat8((t + 2^(19 - e)) >> (20 - e)) with rnd = 2^(19 - e), sh = 20 - e
__device__ __forceinline__ int32_t chz_gain_rail(int32_t r, int32_t m18, int32_t rnd, uint32_t sh)
{
    return chz_sat((__mulhi(r, m18) + rnd) >> sh, -128, 127);
}

// Every thread of the workgroup: the window of outputs [m0, m0 + nloc) of one source - bytes [2 M m0 - 2 Kp, 2 M (m0 +
// nloc)) of [history | this call], made signed - into LDS.
__device__ __forceinline__ void chz_stage_window(const ChzLaunch &a, uint32_t source, uint32_t m0, uint32_t nloc, uint8_t *win)
{
    const uint32_t M = a.m, kp = a.kp;
    const uint8_t *src = a.wide + (size_t)source * a.bytes_per_source;
    const uint8_t *hsrc = a.hist + (size_t)source * 2 * kp;
    const int64_t b0 = 2 * (int64_t)m0 * M - 2 * (int64_t)kp;   // 16-byte aligned, like the history's end
    const uint32_t wbytes = 2 * (nloc * M + kp);
    for (uint32_t i = threadIdx.x * 16; i < wbytes; i += blockDim.x * 16) {
        const int64_t b = b0 + i;
        uint4 v = b < 0 ? *(const uint4 *)(hsrc + 2 * kp + b) : *(const uint4 *)(src + b);
        v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
        *(uint4 *)(win + i) = v;
    }
}

// Signed 16-bit captures (chz_fmt_kernel, iqd_chan_fmt.hip).  Two little-endian samples' dwords w0, w1 = (I lo, I hi, Q lo,
// Q hi) each -> one dword of the high plane (I hi, Q hi of both) and of the low plane (the low bytes - 128, i.e. ^ 0x80).
// Plain shifts and masks: the compiler makes each one v_perm_b32.
__host__ __device__ __forceinline__ uint32_t chz_fmt_hi(uint32_t w0, uint32_t w1)
{
    return ((w0 >> 8) & 0xffu) | ((w0 >> 16) & 0xff00u) | ((w1 << 8) & 0xff0000u) | (w1 & 0xff000000u);
}
__host__ __device__ __forceinline__ uint32_t chz_fmt_lo(uint32_t w0, uint32_t w1)
{
    return ((w0 & 0xffu) | ((w0 >> 8) & 0xff00u) | ((w1 << 16) & 0xff0000u) | ((w1 << 8) & 0xff000000u)) ^ 0x80808080u;
}

// One rail of an S16 output before sat16: (A + 2^15) >> 16 for A = 256 H + Lo' + 128 G, from the accumulators of the high
// sample plane (H: tap planes hlo, hhi), of the low one (Lo': llo, lhi) and the row's coefficient sum G.  H and Lo' fit int32
// like chz_epilogue's A (their 256 hi alone need not: combined modulo 2^32); Lo = Lo' + 128 G need not and is an int64;
// |(Lo + 2^15) >> 8| < 2^25 and its sum with H fit int32 again.  |result| < 2^23.
__host__ __device__ __forceinline__ int32_t chz_fmt_stage_a(int32_t hlo, int32_t hhi, int32_t llo, int32_t lhi, int32_t G)
{
    const int32_t H = (int32_t)((uint32_t)hlo + ((uint32_t)hhi << 8));
    const int32_t Lp = (int32_t)((uint32_t)llo + ((uint32_t)lhi << 8));
    const int64_t Lo = (int64_t)Lp + 128 * (int64_t)G;
    return (H + (int32_t)((Lo + 32768) >> 8)) >> 8;
}

}  // namespace iqd
