// Device pieces of the wideband channelizer, each written once for chz_kernel / chz_scan_kernel (iqd_chan.hip),
// chz_frac_kernel (iqd_chan_frac.hip), chz_survey_kernel (iqd_chan_survey.hip), chz_fmt_kernel (iqd_chan_fmt.hip),
// chz_gain_kernel (iqd_chan_gain.hip) and chz_track_kernel (iqd_chan_track.hip): the B operand read, the epilogue of one output, the window staging, the prologue
// (phasor table, a lane's tile parameters and A operands), the accumulate step, the group walk with its Finish and Sink
// policies, the walkers' block close.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan.h"
#include "iqd_chains.h"

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

// One channel's output at one sample up to the rotation: the two rails' accumulators (lo / hi tap planes) -> stage a and
// rr = ar c + ai s, ri = ai c - ar s, |rr|, |ri| < 2^31
__device__ __forceinline__ void chz_epilogue_rot(int32_t rlo, int32_t rhi, int32_t ilo, int32_t ihi, uint32_t p, int32_t &rr,
                                                 int32_t &ri)
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
    rr = __builtin_amdgcn_sdot2(va, cs, 0, false);                     // ar c + ai s
    ri = __builtin_amdgcn_sdot2(vb, cns, 0, false);                    // ai c - ar s
}

// the whole of it: round, shift, saturate -> two offset-binary bytes
__device__ __forceinline__ uint32_t chz_epilogue(int32_t rlo, int32_t rhi, int32_t ilo, int32_t ihi, uint32_t p,
                                                 int32_t rnd, uint32_t sh)
{
    int32_t rr, ri;
    chz_epilogue_rot(rlo, rhi, ilo, ihi, p, rr, ri);
    const int32_t yr = chz_sat((rr + rnd) >> sh, -128, 127), yi = chz_sat((ri + rnd) >> sh, -128, 127);
    return (uint32_t)(yr + 128) | ((uint32_t)(yi + 128) << 8);
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

// How a window's capture bytes become signed-byte planes: offset binary (^ 0x80), signed bytes as they are, or signed
// 16-bit samples split into a high and a low plane (chz_fmt_hi / chz_fmt_lo).
enum ChzSamples { CHZ_U8, CHZ_S8, CHZ_S16 };

// Every thread of the workgroup: samples [M m0 - Kp, M (m0 + nloc)) of [history | this call] of one source - the window of
// outputs [m0, m0 + nloc) - into LDS, as one plane of 2 (nloc M + Kp) signed bytes at win (CHZ_S16: two, pstride apart).
// A thread moves 16 plane bytes per plane and step (16 B capture bytes, B = a.rail_bytes); the history's end and every
// step are aligned to that, so a step lies on one side of the boundary.
template <ChzSamples F>
__device__ __forceinline__ void chz_stage_window(const ChzLaunch &a, uint32_t source, uint32_t m0, uint32_t nloc, uint8_t *win,
                                                 uint32_t pstride = 0)
{
    constexpr int B = F == CHZ_S16 ? 2 : 1;
    const uint32_t M = a.m, kp = a.kp;
    const size_t hb = (size_t)2 * kp * B;                       // history bytes of one source
    const uint8_t *src = a.wide + (size_t)source * a.bytes_per_source;
    const uint8_t *hend = a.hist + (size_t)source * hb + hb;
    const int64_t s0 = (int64_t)m0 * M - (int64_t)kp;           // first sample of the window, a multiple of 32
    const uint32_t pbytes = 2 * (nloc * M + kp);                // bytes of one plane, a multiple of 64
    for (uint32_t i = threadIdx.x * 16; i < pbytes; i += blockDim.x * 16) {
        const int64_t b = (2 * s0 + i) * B;                     // capture byte of plane byte i
        const uint4 *p = (const uint4 *)(b < 0 ? hend + b : src + b);
        if (F != CHZ_S16) {
            uint4 v = p[0];
            if (F == CHZ_U8) { v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u; }
            *(uint4 *)(win + i) = v;
        } else {
            const uint4 u = p[0], v = p[1];                     // eight samples: (I lo, I hi, Q lo, Q hi) each
            uint4 hi, lo;
            hi.x = chz_fmt_hi(u.x, u.y); hi.y = chz_fmt_hi(u.z, u.w); hi.z = chz_fmt_hi(v.x, v.y); hi.w = chz_fmt_hi(v.z, v.w);
            lo.x = chz_fmt_lo(u.x, u.y); lo.y = chz_fmt_lo(u.z, u.w); lo.z = chz_fmt_lo(v.x, v.y); lo.w = chz_fmt_lo(v.z, v.w);
            *(uint4 *)(win + i) = hi;
            *(uint4 *)(win + pstride + i) = lo;
        }
    }
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

// ---- the pieces every channelizer kernel is made of ----

// every thread of the workgroup: the phasor table into LDS (read after the caller's next barrier)
__device__ __forceinline__ void chz_phasor_to_lds(const ChzLaunch &a, uint32_t *sp)
{
    for (uint32_t i = threadIdx.x; i < CHZ_PHASOR / 4; i += blockDim.x) ((uint4 *)sp)[i] = ((const uint4 *)a.phasor)[i];
}

// Finish of chz_walk (below): chz_epilogue with the gain shifts L of the lane's two channels, shv = 22 - L, rnd = 2^(21 - L)
struct ChzFinish {
    uint32_t shv[2];
    int32_t rnd[2];
    __device__ __forceinline__ uint32_t operator()(const chz_v4i (&acc)[1][2], int i, uint32_t p) const
    {
        return chz_epilogue(acc[0][0][2 * i], acc[0][1][2 * i], acc[0][0][2 * i + 1], acc[0][1][2 * i + 1], p, rnd[i], shv[i]);
    }
};

// A lane's share of one tile: the increments and gain shifts of its two channels (slots 2 g, 2 g + 1), the row it stores
// (slot lane >> 3), the tile's A operands at this lane - in amat, [residues][nq][2 planes] 64 lanes apart - and, for
// NQR > 0 (nq <= NQR, one residue), in registers.  A kernel uses what it needs (the scan walker no inc, the gain walker
// no fin, only the survey ch); params reads them all and leaves the rest to dead-code elimination, which the kernels'
// instruction counts show to happen.
template <int NQR>
struct ChzLaneTile {
    uint32_t inc[2], ch[2], st_ch;
    ChzFinish fin;
    const uint4 *amat;
    chz_v4i A[NQR > 0 ? NQR : 1][2];

    __device__ __forceinline__ void params(const ChzLaunch &a, uint32_t tile, uint32_t residues, bool active)
    {
        const uint32_t lane = threadIdx.x & 63, g = lane >> 4;
        const ChzTile *T = a.tiles + tile;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            inc[i] = T->inc[2 * g + i];
            const uint32_t L = T->shift[2 * g + i];
            fin.shv[i] = 22 - L;
            fin.rnd[i] = 1 << (21 - L);
            ch[i] = T->ch[2 * g + i];
        }
        st_ch = active ? T->ch[lane >> 3] : CHZ_NONE;
        amat = a.amat + (size_t)tile * residues * a.nq * 2 * 64 + lane;
    }
    __device__ __forceinline__ void load_a(uint32_t nq)
    {
        if (NQR > 0) {
#pragma unroll
            for (int q = 0; q < NQR; q++)
                if (q < (int)nq) {
                    A[q][0] = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 0) * 64]);
                    A[q][1] = __builtin_bit_cast(chz_v4i, amat[(q * 2 + 1) * 64]);
                }
        }
    }
};

// The accumulate step: every 64-byte K-chunk q of a pair of accumulator sets - NT = 2 / PLANES 16-output MFMA tiles, each
// on PLANES sample planes pstride apart - and both tap planes: acc[t][s][p] += A[q][p] x B[t][s][q], four independent
// chains.  A: the operands in registers (NQR > 0: nq <= NQR) or am[t], read per chunk (NQR = 0; tiles of one tap set pass
// the same pointer and share the read).  ob(t): LDS byte offset of tile t's B operand at q = 0, a functor that captures
// by value and forms the offset where it is used (an offset kept per tile, or captures by reference, cost chz_kernel and
// chz_fmt_kernel VGPRs).
template <int NQR, int PLANES, class Ob>
__device__ __forceinline__ void chz_accumulate(chz_v4i (&acc)[2 / PLANES][PLANES][2], const uint8_t *win, uint32_t pstride,
                                               const Ob &ob, const chz_v4i (&A)[NQR > 0 ? NQR : 1][2],
                                               const uint4 *const (&am)[2 / PLANES], uint32_t nq)
{
    if (NQR > 0) {
#pragma unroll
        for (int q = 0; q < NQR; q++)
            if (q < (int)nq) {
#pragma unroll
                for (int t = 0; t < 2 / PLANES; t++)
#pragma unroll
                    for (int s = 0; s < PLANES; s++) {
                        const chz_v4i b = chz_b_operand(win + s * pstride, ob(t) + 64 * q);
                        acc[t][s][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[q][0], b, acc[t][s][0], 0, 0, 0);
                        acc[t][s][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[q][1], b, acc[t][s][1], 0, 0, 0);
                    }
            }
    } else {
        for (uint32_t q = 0; q < nq; q++) {
#pragma unroll
            for (int t = 0; t < 2 / PLANES; t++) {
                const chz_v4i alo = __builtin_bit_cast(chz_v4i, am[t][(q * 2 + 0) * 64]);
                const chz_v4i ahi = __builtin_bit_cast(chz_v4i, am[t][(q * 2 + 1) * 64]);
#pragma unroll
                for (int s = 0; s < PLANES; s++) {
                    const chz_v4i b = chz_b_operand(win + s * pstride, ob(t) + 64 * q);
                    acc[t][s][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(alo, b, acc[t][s][0], 0, 0, 0);
                    acc[t][s][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ahi, b, acc[t][s][1], 0, 0, 0);
                }
            }
        }
    }
}

// How chz_walk addresses the 16 outputs of an MFMA tile: as consecutive outputs of the integer decimator (Q = 1 only), or as
// outputs of one residue of a store group (any Q)
enum ChzOffsets { CHZ_CONSECUTIVE, CHZ_PER_RESIDUE };

// outputs of one store group at decimation P / Q (Q = 1: the integer decimator)
constexpr uint32_t chz_group_outputs(uint32_t q) { return q == 1 ? CHZ_GROUP : chz_frac_group(q); }

// The group walk.  One wave: its tile's outputs [m0, m0 + nloc) - m0 a multiple of G = chz_group_outputs(Q), nloc of 32
// (Q = 1) or G - every gstride-th store group from grp0, from the window staged for the wide steps of t0 = m0 / Q on.
// MFMA tile ti of a group is residue rho = ti % Q, the 16 outputs rho + Q (16 (ti / Q) + col): an integer decimator by P
// whose windows start at byte 2 (P t + e_rho + 1), e_rho = ((rho + 1) P - 1) / Q, with the tap set of residue rho (Q = 1:
// 16 consecutive outputs, e = P - 1, one tap set).  2 / PLANES tiles at a time through chz_accumulate; then per tile and
// slot i of the lane - lane (col, g) holds rows 4 g .. 4 g + 3 = channels 2 g, 2 g + 1 (re, im) of output col -
//   fin(acc[t], i, p)       the byte pair of the output from its accumulators and phasor p      (Finish)
//   sink.put(i, jt, pair)   output jt of the group, the lane's channel i                        (Sink)
// sink.begin(m) comes before the step whose outputs start at m, sink.end(a, m, ntl) after the group at m of ntl tiles.
// Sink::UNROLL: the steps of a group are unrolled (the fractional store group, whose tile count is fixed);
// OFS: how the step forms the windows' offsets and the wide sample index (the same numbers either way; see the step).
template <int Q, int NQR, int PLANES, ChzOffsets OFS, class Finish, class Sink>
__device__ __forceinline__ void chz_walk(const ChzLaunch &a, const uint8_t *win, uint32_t pstride, const uint32_t *sp,
                                         const chz_v4i (&A)[NQR > 0 ? NQR : 1][2], const uint4 *amat, const uint32_t (&inc)[2],
                                         uint32_t m0, uint32_t nloc, uint32_t grp0, uint32_t gstride, const Finish &fin, Sink &sink)
{
    static_assert(NQR == 0 || Q == 1, "register-resident A operands are for the integer decimator");
    constexpr uint32_t G = chz_group_outputs(Q), NTG = G / 16, TG = G / Q;   // outputs, MFMA tiles, wide steps t per group
    constexpr int NT = 2 / PLANES;
    static_assert(OFS == CHZ_PER_RESIDUE || Q == 1, "consecutive outputs are the integer decimator's");
    constexpr bool CONSEC = OFS == CHZ_CONSECUTIVE;
    const uint32_t lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const uint32_t P = a.m, nq = a.nq, t0 = m0 / Q;
    const chz_v4i zero = {0, 0, 0, 0};
    for (uint32_t grp = grp0; grp * G < nloc; grp += gstride) {
        const uint32_t ntl = Q == 1 ? min(NTG, (nloc - grp * G) / 16) : NTG;   // Q = 1: 2 or 4
        auto step = [&](uint32_t tp) {
            sink.begin(m0 + grp * G + (Q == 1 ? 16 * tp : 0));
            chz_v4i acc[NT][PLANES][2];
            uint32_t e[NT], tt[NT];
            const uint4 *am[NT];
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int s = 0; s < PLANES; s++) acc[t][s][0] = acc[t][s][1] = zero;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const uint32_t rho = (tp + t) % Q;
                e[t] = ((rho + 1) * P - 1) / Q;
                tt[t] = grp * TG + 16 * ((tp + t) / Q) + col;            // wide step within the window
                am[t] = amat + (size_t)rho * nq * 2 * 64;
            }
            // The windows' byte offsets and the outputs' wide sample n, two ways to the same numbers: consecutive outputs
            // (one base, a uniform step per tile) or per residue.  One form for all costs chz_kernel, chz_fmt_kernel and
            // chz_gain_kernel VGPRs at Q = 1 in the residues' form, and chz_survey_kernel<1, 8> in the other: the kernel says
            // which (OFS).
            // Per residue with A in registers (that kernel) the offset is formed here, once, not per unrolled chunk: that
            // cost it 2.9 % of its time; everywhere else forming it where it is used is what keeps the register counts.
            const uint32_t obase = 2 * P * (grp * G + 16 * tp + col + 1) + 16 * g;
            uint32_t obv[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) obv[t] = 2 * (P * tt[t] + e[t] + 1) + 16 * g;
            const auto ob = [=](int t) {
                if (CONSEC) return obase + 2 * P * 16 * t;
                return NQR > 0 ? obv[t] : 2 * (P * tt[t] + e[t] + 1) + 16 * g;
            };
            chz_accumulate<NQR, PLANES>(acc, win, pstride, ob, A, am, nq);
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const uint32_t rho = (tp + t) % Q;
                const uint32_t jt = rho + Q * (16 * ((tp + t) / Q) + col);   // output within the group
                const uint32_t n32 = a.nbase + (CONSEC ? (m0 + grp * G + jt) * P + P - 1 : (t0 + tt[t]) * P + e[t]);   // mod 2^32
#pragma unroll
                for (int i = 0; i < 2; i++) sink.put(i, jt, fin(acc[t], i, sp[(n32 * inc[i]) >> 20]));
            }
        };
        if constexpr (Sink::UNROLL) {
#pragma unroll
            for (uint32_t tp = 0; tp < NTG; tp += NT) step(tp);
        } else {
            for (uint32_t tp = 0; tp < ntl; tp += NT) step(tp);
        }
        sink.end(a, m0 + grp * G, ntl);
    }
}

// Sink of chz_walk: the byte pairs into the wave's LDS staging row of 8 channels x 2 G bytes, then per group one 16-byte
// store per lane and 128 bytes of a row (8 lanes write one channel's 128 contiguous bytes: whole sectors; Q = 1: the
// row's pieces below the group's ntl tiles).  MAG: also sums SignalDetector's magnitude of the bytes this lane stores
// (the walkers' squelch).
template <int Q, bool MAG>
struct ChzRowSink {
    static constexpr bool UNROLL = Q > 1;
    static constexpr uint32_t G = chz_group_outputs(Q);
    uint8_t *stage;
    uint32_t st_ch, mag;
    __device__ __forceinline__ void begin(uint32_t) {}
    __device__ __forceinline__ void put(int i, uint32_t jt, uint32_t v)
    {
        const uint32_t g = (threadIdx.x & 63) >> 4;
        *(uint16_t *)(stage + (2 * g + i) * (2 * G) + 2 * jt) = (uint16_t)v;
    }
    __device__ __forceinline__ void end(const ChzLaunch &a, uint32_t m, uint32_t ntl)
    {
        const uint32_t lane = threadIdx.x & 63, st_cl = lane >> 3, st_piece = lane & 7;
        chz_wave_fence();
        if (st_ch != CHZ_NONE && (Q > 1 || st_piece * 8 < ntl * 16)) {
#pragma unroll
            for (uint32_t s = 0; s < 2 * G / 128; s++) {
                const uint4 v = *(const uint4 *)(stage + st_cl * (2 * G) + 128 * s + 16 * st_piece);
                *(uint4 *)(a.out + (size_t)st_ch * a.out_row + 2 * (size_t)m + 128 * s + 16 * st_piece) = v;
                if (MAG)
                    mag += magnitude2(v.x ^ 0x80808080u) + magnitude2(v.y ^ 0x80808080u) + magnitude2(v.z ^ 0x80808080u) +
                           magnitude2(v.w ^ 0x80808080u);
            }
        }
        chz_wave_fence();
    }
};

// The walkers' block close (chz_scan_kernel, chz_gain_kernel).  magsum: [2][CHZ_WAVES * 8] sums in LDS by block parity, one
// per (tile of the workgroup, slot).  chz_block_open zeroes block b's before the barrier that opens the block;
// chz_block_close adds the lane's magnitude over the channel's 8 storing lanes and, in the channel's owner lane (lane 8 l
// for slot l), over the tile's waves, and returns where the owner reads the block's sum after the barrier inside.
__device__ __forceinline__ void chz_block_open(uint32_t *magsum, uint32_t b)
{
    if (threadIdx.x < CHZ_WAVES * 8) magsum[(b & 1) * CHZ_WAVES * 8 + threadIdx.x] = 0;
}
__device__ __forceinline__ const uint32_t *chz_block_close(uint32_t *magsum, uint32_t b, uint32_t tl, uint32_t mag, bool owner)
{
    mag += (uint32_t)__shfl_xor((int)mag, 1);
    mag += (uint32_t)__shfl_xor((int)mag, 2);
    mag += (uint32_t)__shfl_xor((int)mag, 4);
    uint32_t *ms = magsum + (b & 1) * CHZ_WAVES * 8 + tl * 8 + ((threadIdx.x & 63) >> 3);
    if (owner) atomicAdd(ms, mag);
    __syncthreads();
    return ms;
}

}  // namespace iqd
