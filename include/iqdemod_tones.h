/* libiqdemod add-on: the PCM tone bank (iqd_tones_*).  Which of T given tones - CTCSS, DTMF, a 1750 Hz burst, selcall - is in
 * every channel's PCM, frame by frame, on the engine's stream behind the call that writes the PCM, with no host trip.
 *
 * An add-on: the functions live in the same libiqdemod.so, but this header, IQD_TONES_ABI_VERSION and the Python
 * binding's table (rtlsdrdiags_amd/tones.py: PROTOTYPES) are its own; include/iqdemod.h and IQD_ABI_VERSION do not know it.
 *
 * Every quantity is an integer and every step is fixed below, so results are exact (tests/tones_model.py is written from
 * this text).  >> is an arithmetic shift (floor); sums and products are in unbounded integers unless a width is given.
 *
 *   input     pcm_dev[n_channels][row_stride] int16; row c holds m_c valid samples from its start: m_c = n if count_dev is
 *             NULL, else min(count_dev[c], n) (a squelch-gated accept's packed rows and pcm_count fit as they are).
 *             0 <= n <= row_stride <= 2^31 - 1.  Rows need 2-byte alignment only.  A channel's samples of successive
 *             calls are one stream.
 *   frames    a frame is L consecutive samples of a channel's stream; frames do not overlap and follow each other without
 *             a gap.  L is a multiple of 32, 32 <= L <= 8192.  Frames straddle calls: per channel the object carries the
 *             open frame (its samples so far; `fill` of them, 0 <= fill < L) and the decision state below.
 *             iqd_tones_reset clears both for every channel; create starts cleared.
 *   tones     T tones, 1 <= T <= 64, each a phase increment d_t (uint32: cycles per sample x 2^32).  Duplicates are legal.
 *             iqd_tones_phase_inc(freq_mhz, rate_hz, &d): d = floor((freq_mhz 2^32 + 500 rate_hz) / (1000 rate_hz)), the
 *             frequency in millihertz; IQD_EINVAL for d NULL, rate_hz = 0 or freq_mhz >= 500 rate_hz.  Host only.
 *   window    w[0..L) int16, |w[n]| <= 32767 (-32768 is refused).  NULL selects the default
 *                 w[n] = (32767 - Pc[floor((2 n + 1) 2048 / L)]) >> 2
 *             - a Hann window with a half-sample offset, 0 <= w <= 16383; the floor is the rule for every L (it only matters
 *             for L = 8192, where (2 n + 1) / 4 is no integer).  iqd_tones_default_window(L, w) writes it; host only.
 *   coeffs    P[i] = (Pc[i], Ps[i]) is iqd_channelizer_phasor_table, 4096 entries.  With n counted from the FRAME's first
 *             sample: i_t(n) = ((n d_t) mod 2^32) >> 20,
 *                 c_t[n] = (w[n] Pc[i_t(n)] + 2^14) >> 15,     s_t[n] = (w[n] Ps[i_t(n)] + 2^14) >> 15.
 *             Built once at create on the host ([T][L] int16 pairs, 2 MiB at most).
 *   per frame with x[0..L) the frame's samples:
 *                 Ar_t = sum c_t[n] x[n],  Ai_t = sum s_t[n] x[n]                      (|A| < 2^44)
 *                 ar_t = (Ar_t + 2^15) >> 16,  ai_t likewise,  p_t = ar_t^2 + ai_t^2   (uint64, < 2^57)
 *                 E = sum x[n]^2                                                       (uint64)
 *             best = the lowest t with the largest p; second = the lowest t != best with the largest p among the others.
 *             T = 1: second = 0xffffffff and p_second = 0.
 *   hit       iff  p_best >= min_power  and  256 p_best >= ratio_q8 p_second  and  256 p_best >= energy_q8 E
 *             (products in unbounded integers).  256 <= ratio_q8 <= 65535, 0 <= energy_q8 <= 2^20, min_power any uint64.
 *             f = hit ? best : -1.  (Silence: every p is 0, best = 0, and it is a hit only if min_power is 0.)
 *   decision  per channel, frame by frame in stream order, on the state tone (-1 = none), cand, run, miss
 *             (cleared: tone = cand = -1, run = miss = 0):
 *               1. if f >= 0 and f == cand: run += 1 (saturating at 2^32 - 1); else cand = f, run = (f >= 0 ? 1 : 0)
 *               2. if tone >= 0: if f == tone: miss = 0; else miss += 1;
 *                                if miss > hold: tone = -1, miss = 0, flag IQD_TONES_F_CLOSED
 *               3. if tone < 0 and cand >= 0 and run >= open: tone = cand, miss = 0, flag IQD_TONES_F_OPENED
 *             1 <= open <= 255, 0 <= hold <= 255.  A frame may set both flags: a switch of tone.
 *   output    n_frames_dev[n_channels] uint32: the frames this call completed, k_c = floor((fill_c + m_c) / L).
 *             frames_dev[n_channels][F] iqd_tones_frame, F = iqd_tones_max_frames(t, n) = floor((n + L - 1) / L): the k_c
 *             frames in stream order; `tone` is the tone in force after the frame.
 *             power_dev[n_channels][F][T] uint64, optional (NULL: not written): every p_t.
 *             Records and power rows from k_c on are all-zero bytes: every array is defined in full after a call.
 *             n = 0 is no error: it writes the zero counts (F = 0: the other arrays are empty and may be any non-NULL
 *             aligned pointer) and moves no state.
 *   state     iqd_tones_get_state(t, ch, &s): one channel's tone, cand, run, miss and fill; synchronises.
 *   calls     iqd_tones_run_device: device pointers, frames_dev and power_dev 16-byte aligned, pcm_dev 2-byte, count_dev and
 *             n_frames_dev 4-byte; queued on the engine's stream (two launches for n > 0 whatever n, L and the frame count
 *             are; one for n = 0), returns once queued.  iqd_tones_run: the same on host pointers, staged; synchronises.
 *   refusals  IQD_EINVAL with a message naming the argument, before anything is allocated or queued, the stream intact.
 *             create: e NULL (no message), out NULL, cfg NULL, abi_version, n_channels (1 .. 2^20), frame_len, n_tones,
 *             phase_inc NULL, a window entry of -32768, ratio_q8, energy_q8, open, hold, a reserved word, in this order.
 *             run / run_device: t NULL (no message); e not t's engine; then NULLs in argument order (pcm, n_frames, frames;
 *             count and power may be NULL); then n > row_stride, row_stride > 2^31 - 1 (n first); then, run_device only,
 *             alignment in argument order. */
#ifndef IQDEMOD_TONES_H
#define IQDEMOD_TONES_H

#include "iqdemod.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IQD_TONES_ABI_VERSION 1

#define IQD_TONES_F_OPENED 1u
#define IQD_TONES_F_CLOSED 2u
#define IQD_TONES_NONE 0xffffffffu   /* iqd_tones_frame.second for T = 1 */

typedef struct iqd_tones iqd_tones_t;

typedef struct iqd_tones_config {
    uint32_t abi_version;        /* IQD_TONES_ABI_VERSION */
    uint32_t n_channels;
    uint32_t frame_len;          /* L */
    uint32_t n_tones;            /* T */
    const uint32_t *phase_inc;   /* [T] */
    const int16_t *window;       /* [L], or NULL for the default */
    uint64_t min_power;
    uint32_t ratio_q8;
    uint32_t energy_q8;
    uint32_t open;
    uint32_t hold;
    uint32_t reserved[4];        /* 0 */
} iqd_tones_config;              /* 72 bytes */

typedef struct iqd_tones_frame {
    uint64_t energy;
    uint64_t p_best;
    uint64_t p_second;
    uint32_t best;
    uint32_t second;
    int32_t tone;                /* in force after the frame; -1 = none */
    uint32_t flags;              /* IQD_TONES_F_* */
} iqd_tones_frame;               /* 40 bytes */

typedef struct iqd_tones_state {
    int32_t tone;
    int32_t cand;
    uint32_t run;
    uint32_t miss;
    uint32_t fill;               /* samples in the open frame */
    uint32_t reserved[3];        /* 0 */
} iqd_tones_state;               /* 32 bytes */

int iqd_tones_create(iqd_t *e, const iqd_tones_config *cfg, iqd_tones_t **out);
void iqd_tones_destroy(iqd_tones_t *t);
int iqd_tones_reset(iqd_tones_t *t);
size_t iqd_tones_max_frames(const iqd_tones_t *t, size_t n);
int iqd_tones_run_device(iqd_t *e, iqd_tones_t *t, const int16_t *pcm_dev, size_t row_stride, const uint32_t *count_dev, size_t n,
                         uint32_t *n_frames_dev, iqd_tones_frame *frames_dev, uint64_t *power_dev);
int iqd_tones_run(iqd_t *e, iqd_tones_t *t, const int16_t *pcm, size_t row_stride, const uint32_t *count, size_t n,
                  uint32_t *n_frames, iqd_tones_frame *frames, uint64_t *power);
int iqd_tones_get_state(iqd_tones_t *t, uint32_t channel, iqd_tones_state *state);

/* host only, no GPU */
int iqd_tones_phase_inc(uint64_t freq_mhz, uint32_t rate_hz, uint32_t *d);
int iqd_tones_default_window(uint32_t frame_len, int16_t *window);
int iqd_tones_ctcss(uint32_t freq_mhz[50]);   /* the 50 standard CTCSS tones, 67.0 .. 254.1 Hz, in millihertz, rising */
int iqd_tones_dtmf(uint32_t freq_mhz[8]);     /* 697, 770, 852, 941, 1209, 1336, 1477, 1633 Hz in millihertz */

#ifdef __cplusplus
}
#endif
#endif
