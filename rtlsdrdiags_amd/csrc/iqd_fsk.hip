// PCM packet decoder (include/iqdemod_fsk.h; what the host passes: iqd_fsk.h).  Two launches per call, whatever n, the channel
// count and the number of frames are.
//
// fsk_decide_kernel   parallel over samples: a workgroup of four waves takes FSK_TILE consecutive samples of one channel (the
//                     other tiles and the channels past 65535 by stride loops).  It stages the tile and the W - 1 samples in
//                     front of it in LDS - one 2-byte load per sample, consecutive lanes on consecutive samples, so the rows
//                     need no more alignment; in front of the call's first sample stand the W - 1 samples the channel
//                     carries - runs the four W-tap correlators (coefficients from the kernel's arguments: scalar loads, the
//                     tap index is uniform) in int32, forms soft in int64, and a wave's ballot over its 64 samples gives two
//                     decision words.  Samples from m_c on decide 0; words past ceil(m_c / 32) may stay unwritten, the walk
//                     does not read them.
// fsk_walk_kernel     one wave per channel.  The 64 lanes zero the channel's records, bytes and bit words, fetch the bit
//                     buffer into LDS and move the carried samples on; then lane 0 walks the decision words in stream order
//                     through the bit clock, NRZI, the deframer and the CRC, and writes the bit words, the records, the
//                     payload bytes, the counts and the state.
// No atomics; the result cannot depend on the launch shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_fsk.h"

namespace iqd {

constexpr uint32_t FSK_BUF_WORDS = FSK_BUF_BYTES / 4;
constexpr uint32_t FSK_DEC_WORDS = 2048;   // decision words the walk holds in LDS at a time: 65536 samples

__device__ __forceinline__ uint32_t fsk_count(const FskLaunch &a, uint32_t ch) { return a.count ? min(a.count[ch], a.n) : a.n; }

__global__ __launch_bounds__(FSK_TILE) void fsk_decide_kernel(const FskLaunch a)
{
    __shared__ int16_t x[FSK_TILE + FSK_MAX_W];   // x[i]: the call's sample t0 - (W - 1) + i
    const uint32_t tid = threadIdx.x, W = a.W;
    for (uint32_t ch = blockIdx.y; ch < a.n_channels; ch += gridDim.y) {
        const uint32_t m = fsk_count(a, ch);
        const int16_t *row = a.pcm + (size_t)ch * a.row_stride, *hist = a.hist + (size_t)ch * FSK_HIST;
        for (uint64_t t0 = (uint64_t)blockIdx.x * FSK_TILE; t0 < m; t0 += (uint64_t)gridDim.x * FSK_TILE) {
            for (uint32_t i = tid; i < FSK_TILE + W - 1; i += FSK_TILE) {
                const int64_t p = (int64_t)t0 + i - (int64_t)(W - 1);
                x[i] = p < 0 ? hist[(int64_t)(W - 1) + p] : p < (int64_t)m ? row[p] : (int16_t)0;
            }
            __syncthreads();
            int32_t mr = 0, mi = 0, sr = 0, si = 0;
            for (uint32_t k = 0; k < W; k++) {
                const int32_t v = x[tid + k];
                mr += a.coef[0][k] * v;
                mi += a.coef[1][k] * v;
                sr += a.coef[2][k] * v;
                si += a.coef[3][k] * v;
            }
            const int64_t soft = (int64_t)mr * mr + (int64_t)mi * mi - (int64_t)sr * sr - (int64_t)si * si;
            const uint64_t j = t0 + tid;
            const uint64_t b = __ballot(j < m && soft > 0);
            if ((tid & 63) == 0) {
                const uint64_t w = j >> 5;
                uint32_t *dec = a.dec + (size_t)ch * a.Dw;
                if (w < a.Dw) dec[w] = (uint32_t)b;
                if (w + 1 < a.Dw) dec[w + 1] = (uint32_t)(b >> 32);
            }
            __syncthreads();   // the next tile reuses x
        }
    }
}

__device__ __forceinline__ uint32_t fsk_byte(const uint32_t *buf, uint32_t i) { return (buf[i >> 2] >> (8 * (i & 3))) & 255u; }

// Lane 0's walk over one channel: what it carries in registers, and what one raw bit does
struct FskWalk {
    const FskLaunch &a;
    uint32_t *buf, *frames, *bits;   // the bit buffer (LDS), the channel's records and bit words
    uint8_t *bytes;
    uint64_t samples;                // the stream index of the call's first sample
    uint32_t ph, prev, last, ones, in_frame, nbits, bad, total;
    uint32_t nb, nf, off, word;

    // The raw bit d, emitted at the call's sample jb + i - 1 where i is the k-th carry of a run that began at jb with the
    // phase ph0: i = ceil((k 2^32 - ph0) / b) (k = 0: at jb itself).  The division is done where a frame closes only.
    __device__ __forceinline__ void emit(uint32_t d, uint32_t jb, uint32_t k, uint32_t ph0)
    {
        uint32_t bit = d;
        if (a.nrzi) { bit = d == last; last = d; }
        word |= bit << (nb & 31);
        nb++;
        if ((nb & 31) == 0) {
            if (bits && (nb >> 5) - 1 < a.Bw) bits[(nb >> 5) - 1] = word;
            word = 0;
        }
        bool append = false;
        if (bit) {
            ones = min(ones + 1, 7u);
            if (ones == 7) in_frame = 0;
            else append = in_frame;
        } else {
            const uint32_t o = ones;
            ones = 0;
            if (o == 6) {
                const int32_t Lb = (int32_t)nbits - 7;
                if (in_frame && Lb >= (int32_t)(8 * a.min_len) && (Lb & 7) == 0) close((uint32_t)Lb >> 3, jb, k, ph0);
                in_frame = 1;
                nbits = 0;
            } else if (o != 5) {
                append = in_frame;
            }
        }
        if (append) {
            if ((nbits & 31) == 0) buf[nbits >> 5] = bit;
            else buf[nbits >> 5] |= bit << (nbits & 31);
            nbits++;
            if (nbits > 8 * a.max_len + 7) in_frame = 0;
        }
    }

    // a frame of B bytes stands in the buffer: the CRC, then the record and the payload, or the bad_fcs count
    __device__ __noinline__ void close(uint32_t B, uint32_t jb, uint32_t k, uint32_t ph0)
    {
        uint32_t crc = 0xffffu;
        for (uint32_t i = 0; i + 2 < B; i++) {
            crc ^= fsk_byte(buf, i);
            for (int q = 0; q < 8; q++) crc = (crc >> 1) ^ (0x8408u & (0u - (crc & 1u)));
        }
        crc ^= 0xffffu;
        const uint32_t fcs = fsk_byte(buf, B - 2) | fsk_byte(buf, B - 1) << 8;
        if (crc != fcs) {
            bad += bad != 0xffffffffu;
            return;
        }
        if (nf < a.F && off + (B - 2) <= a.Bc) {   // the header's bounds hold both; never past the rows
            const uint64_t i = k ? (((uint64_t)k << 32) - ph0 + a.baud_inc - 1) / a.baud_inc - 1 : 0;
            const uint64_t end = samples + jb + i;
            uint32_t *r = frames + (size_t)nf * 6;
            r[0] = (uint32_t)end; r[1] = (uint32_t)(end >> 32);
            r[2] = off; r[3] = B - 2; r[4] = fcs; r[5] = 0;
            for (uint32_t q = 0; q + 2 < B; q++) bytes[off + q] = (uint8_t)fsk_byte(buf, q);
            off += B - 2;
            nf++;
        }
        total += total != 0xffffffffu;
    }
};

// The walk goes from transition to transition: between two the clock is closed-form - a run of r equal decisions emits
// floor((ph + r b) / 2^32) bits - and the next transition is found with ctz on the decision words, which the wave fetches into
// LDS FSK_DEC_WORDS at a time (a run cut at such a boundary, like one cut by a call, gives the same bits: the closed form adds
// up and the second piece begins without a transition).
__global__ __launch_bounds__(64) void fsk_walk_kernel(const FskLaunch a)
{
    __shared__ uint32_t buf[FSK_BUF_WORDS];
    __shared__ uint32_t dw[FSK_DEC_WORDS];
    __shared__ uint32_t keep;
    const uint32_t ch = blockIdx.x, lane = threadIdx.x, W = a.W;
    const FskState st = a.state[ch];
    const uint32_t m = fsk_count(a, ch);

    uint32_t *frames = a.frames + (size_t)ch * a.F * 6;
    uint8_t *bytes = a.bytes + (size_t)ch * a.Bc;
    uint32_t *bits = a.bits ? a.bits + (size_t)ch * a.Bw : nullptr;
    for (uint32_t i = lane; i < a.F * 6; i += 64) frames[i] = 0;
    for (uint32_t i = lane; i < a.Bc / 16; i += 64) ((uint4 *)bytes)[i] = uint4{0, 0, 0, 0};
    if (bits)
        for (uint32_t i = lane; i < a.Bw; i += 64) bits[i] = 0;

    uint32_t *gbuf = a.buf + (size_t)ch * FSK_BUF_WORDS;
    for (uint32_t i = lane; i < min((st.nbits + 31) / 32, FSK_BUF_WORDS); i += 64) buf[i] = gbuf[i];

    // the carried samples: the last W - 1 of (what was carried, then the call's m)
    int16_t *hist = a.hist + (size_t)ch * FSK_HIST;
    int16_t hv = 0;
    if (lane < W - 1 && m) {
        const uint64_t idx = (uint64_t)lane + m;
        hv = idx < W - 1 ? hist[idx] : a.pcm[(size_t)ch * a.row_stride + (idx - (W - 1))];
    }
    __syncthreads();   // the zeros are behind, the old carried samples are read
    if (lane < W - 1 && m) hist[lane] = hv;

    FskWalk s{a, buf, frames, bits, bytes, st.samples, st.ph, st.prev, st.last, st.ones, st.in_frame, st.nbits, st.bad_fcs, st.frames_total,
              0, 0, 0, 0};
    const uint32_t b = a.baud_inc, g = b >> a.loop_shift;
    const uint32_t *dec = a.dec + (size_t)ch * a.Dw;
    for (uint32_t c0 = 0; c0 < m; c0 += 32 * FSK_DEC_WORDS) {   // (32 FSK_DEC_WORDS divides 2^32: c0 cannot wrap below m)
        const uint32_t lim = (uint32_t)min((uint64_t)m, (uint64_t)c0 + 32 * FSK_DEC_WORDS);
        __syncthreads();   // lane 0 is through with the words before
        for (uint32_t i = lane; i < (lim - c0 + 31) / 32; i += 64) dw[i] = dec[c0 / 32 + i];
        __syncthreads();
        if (lane == 0) for (uint32_t j = c0; j < lim;) {
            const uint32_t d = (dw[(j - c0) >> 5] >> (j & 31)) & 1u;
            uint32_t end = j;   // the run's end: the first sample from j on that decides otherwise, or lim
            for (;;) {
                const uint32_t left = 32 - (end & 31), diff = (dw[(end - c0) >> 5] ^ (0u - d)) >> (end & 31);
                const uint32_t z = diff ? min((uint32_t)__builtin_ctz(diff), left) : left;
                end += z;
                if (z < left || end >= lim) break;
            }
            end = min(end, lim);
            if (d != s.prev) {
                s.prev = d;
                s.ph = s.ph < 0x80000000u ? s.ph + g : s.ph - g;
            }
            const uint32_t ph0 = s.ph;
            const uint64_t tot = (uint64_t)ph0 + (uint64_t)(end - j) * b;   // below 2^63
            for (uint32_t k = 1; k <= (uint32_t)(tot >> 32); k++) s.emit(d, j, k, ph0);
            s.ph = (uint32_t)tot;
            j = end;
        }
    }
    if (lane == 0) {
        if (bits && (s.nb & 31) && (s.nb >> 5) < a.Bw) bits[s.nb >> 5] = s.word;
        FskState o;
        o.samples = st.samples + m;
        o.ph = s.ph; o.prev = s.prev; o.last = s.last; o.ones = s.ones; o.in_frame = s.in_frame; o.nbits = s.nbits;
        o.bad_fcs = s.bad; o.frames_total = s.total;
        a.state[ch] = o;
        a.n_bits[ch] = s.nb;
        a.n_frames[ch] = s.nf;
        keep = min((s.nbits + 31) / 32, FSK_BUF_WORDS);
    }
    __syncthreads();
    for (uint32_t i = lane; i < keep; i += 64) gbuf[i] = buf[i];
}

static bool fsk_launch_ok(const FskLaunch &a)
{
    return a.n_channels >= 1 && a.n_channels <= (1u << 20) && a.W >= FSK_MIN_W && a.W <= FSK_MAX_W && a.max_len <= FSK_MAX_LEN &&
           a.min_len >= 3 && a.min_len <= a.max_len && a.loop_shift >= 1 && a.loop_shift <= 8 && a.n <= FSK_MAX_N &&
           a.row_stride <= FSK_MAX_N && a.n <= a.row_stride && a.Dw == (a.n + 31) / 32 && a.Bc % 16 == 0;
}

hipError_t launch_fsk_decide(const FskLaunch &a, hipStream_t s)
{
    if (!fsk_launch_ok(a) || a.n == 0) return hipErrorInvalidValue;
    const uint32_t gy = min(a.n_channels, 65535u);
    const uint32_t gx = min((a.n + FSK_TILE - 1) / FSK_TILE, max(1u, (1u << 23) / gy));   // below 2^32 threads in all
    hipLaunchKernelGGL(fsk_decide_kernel, dim3(gx, gy), dim3(FSK_TILE), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fsk_walk(const FskLaunch &a, hipStream_t s)
{
    if (!fsk_launch_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fsk_walk_kernel, dim3(a.n_channels), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace iqd
