/* libiqdemod add-on: the PCM packet decoder (iqd_fsk_*).  The audio-FSK bits (Bell 202: APRS / AX.25 packet, telemetry) and
 * the HDLC frames in every channel's PCM, on the engine's stream behind the call that writes the PCM, with no host trip.
 *
 * An add-on like the tone bank: the functions live in the same libiqdemod.so, but this header, IQD_FSK_ABI_VERSION and the
 * Python binding's table (rtlsdrdiags_amd/fsk.py: PROTOTYPES) are its own; include/iqdemod.h, IQD_ABI_VERSION and
 * include/iqdemod_tones.h do not know it.
 *
 * Every quantity is an integer and every step is fixed below, so results are exact (tests/fsk_model.py is written from this
 * text).  >> is an arithmetic shift (floor); sums and products are in unbounded integers unless a width is given.
 *
 *   input     pcm_dev[n_channels][row_stride] int16; row c holds m_c valid samples from its start: m_c = n if count_dev is
 *             NULL, else min(count_dev[c], n).  0 <= n <= row_stride <= 2^31 - 1.  Rows need 2-byte alignment only.  A
 *             channel's samples of successive calls are one stream x[j], j a uint64 counted from create / reset; x[j] = 0 for
 *             j < 0.  iqd_fsk_reset clears every channel's state; create starts cleared.
 *   config    corr_len W (2 .. 64); mark_inc, space_inc (any uint32: cycles per sample x 2^32; a raw 1 is `mark`);
 *             baud_inc b (bits per sample x 2^32, 2^20 <= b < 2^31); loop_shift (1 .. 8); flags (IQD_FSK_NRZI, every other
 *             bit refused); window w[0..W) int16 with |w| <= 32512, NULL = 32512 throughout; 3 <= min_len <= max_len <= 1024,
 *             the bytes of a frame with its two FCS bytes.
 *             iqd_fsk_phase_inc(freq_mhz, rate_hz, &d): d = floor((freq_mhz 2^32 + 500 rate_hz) / (1000 rate_hz)), the
 *             frequency (or the baud rate) in thousandths; IQD_EINVAL for d NULL, rate_hz = 0 or freq_mhz >= 500 rate_hz.
 *             iqd_fsk_afsk1200(rate_hz, &cfg) fills 1200 Hz (mark) / 2200 Hz (space), 1200 baud, W = 8, loop_shift 3, NRZI,
 *             min_len 17, max_len 512, window NULL, abi_version; n_channels is left 0 for the caller.  IQD_EINVAL for cfg NULL
 *             or a rate at which one of the three has no increment in range.  Both host only.
 *   coeffs    P[i] = (Pc[i], Ps[i]) is iqd_channelizer_phasor_table, 4096 entries.  For k in [0, W), the phase counted from
 *             the WINDOW's first sample, with d = mark_inc:  i = ((k d) mod 2^32) >> 20,
 *                 cm[k] = (w[k] Pc[i] + 2^22) >> 23,      sm[k] = (w[k] Ps[i] + 2^22) >> 23
 *             and cs, ss likewise from space_inc.  |w| <= 32512 puts every coefficient in -127 .. 127, so an int32
 *             accumulator is exact: |sum| <= 64 x 127 x 32768 < 2^28.
 *   decision  per sample j:  Mr = sum_k cm[k] x[j - W + 1 + k], Mi (sm), Sr (cs), Si (ss) likewise;
 *                 soft = Mr^2 + Mi^2 - Sr^2 - Si^2   (int64, |soft| < 2^57);   d = 1 iff soft > 0  (silence: 0).
 *   bit clock per channel prev and ph (uint32), cleared to 0.  Per sample, in this order, with g = b >> loop_shift:
 *               1. if d != prev: prev = d; then if ph < 2^31: ph += g, else ph -= g  (neither can wrap)
 *               2. ph = (ph + b) mod 2^32; on a carry the raw bit r = d is emitted at sample j.
 *   NRZI      with IQD_FSK_NRZI: bit = (r == last) ? 1 : 0, then last = r (cleared to 0); without: bit = r.
 *   HDLC      per channel ones (0 .. 7), in_frame, nbits and a bit buffer of 8 max_len + 8 bits, all cleared.  Per bit:
 *               bit 1:  ones = min(ones + 1, 7); if ones == 7: in_frame = 0 (an abort); else if in_frame: append 1
 *               bit 0:  o = ones, ones = 0;  o == 5: a stuffed zero, dropped;
 *                       o == 6: a flag: close if in_frame (below); then in_frame = 1, nbits = 0;
 *                       otherwise: if in_frame: append 0
 *               append: buffer bit nbits = the bit, nbits += 1; then if nbits > 8 max_len + 7: in_frame = 0.
 *             close:  Lb = nbits - 7 as a signed number (the flag's leading 0 and six 1s were appended).  The frame stands
 *                     only if Lb >= 8 min_len and Lb mod 8 == 0; anything else is dropped silently.  Byte i has bit k =
 *                     buffer bit 8 i + k (LSB first), B = Lb / 8 bytes.  The FCS is CRC-16/X.25 - reflected polynomial 0x8408,
 *                     init 0xffff, final xor 0xffff - over bytes 0 .. B - 3, compared with byte[B - 2] | byte[B - 1] << 8.
 *                     Equal: a frame is emitted (a record, and bytes 0 .. B - 3 as its payload; frames_total += 1,
 *                     saturating).  Unequal: bad_fcs += 1, saturating at 2^32 - 1; no record.
 *   sizes     maxbits(n) = floor(n (b + (b >> loop_shift)) / 2^32) + 1, and maxbits(0) = 0: no call emits more bits.
 *                 F  = iqd_fsk_max_frames(t, n)    = floor(maxbits / (8 min_len + 8)) + 1, and 0 for n = 0
 *                 Bw = iqd_fsk_max_bit_words(t, n) = ceil(maxbits / 32)
 *                 Bc = iqd_fsk_max_bytes(t, n)     = max_len + floor(maxbits / 8) rounded up to a multiple of 16, 0 for n = 0
 *             (they take n, not the counts; t NULL gives 0).
 *   output    n_bits_dev[n_channels] uint32: the bits emitted in this call.
 *             bits_dev[n_channels][Bw] uint32, optional (NULL: not written): the bits after NRZI, bit i of the call in word
 *             i / 32 at position i mod 32.
 *             n_frames_dev[n_channels] uint32: the frames emitted in this call.
 *             frames_dev[n_channels][F] iqd_fsk_frame, in stream order: end_sample = the j at which the closing flag's last
 *             bit was emitted; offset into the channel's byte row; len = B - 2, the payload without the FCS; fcs = the
 *             received FCS (16 bits); flags = 0.
 *             bytes_dev[n_channels][Bc] uint8: the call's payloads back to back (offset of the first = 0).
 *             Everything past what a call used - bit words, records, bytes - is zero bytes: every array is defined in full
 *             after a call.  n = 0 is no error: it writes the zero counts (the other arrays are empty and may be any non-NULL
 *             aligned pointer) and moves no state.
 *   state     iqd_fsk_get_state(t, ch, &s): one channel's samples (the j of its next sample), ph, prev, last, ones, in_frame,
 *             nbits, bad_fcs and frames_total; synchronises.
 *   calls     iqd_fsk_run_device: device pointers; pcm_dev 2-byte aligned, count_dev, n_bits_dev, bits_dev and n_frames_dev
 *             4-byte, frames_dev 8-byte, bytes_dev 16-byte; queued on the engine's stream - two launches for n > 0 whatever
 *             n, the channel count and the frames are, one for n = 0 - and returns once queued.  iqd_fsk_run: the same on host
 *             pointers, staged; synchronises.
 *   refusals  IQD_EINVAL with a message naming the argument, before anything is allocated or queued, the stream intact.
 *             create: e NULL (no message), out NULL, cfg NULL, abi_version, n_channels (1 .. 2^20), corr_len, baud_inc,
 *             loop_shift, flags, a window entry beyond +-32512, min_len, max_len, a reserved word, in this order.
 *             run / run_device: t NULL (no message); e not t's engine; then NULLs in argument order (pcm, n_bits, n_frames,
 *             frames, bytes; count and bits may be NULL); then n > row_stride, row_stride > 2^31 - 1 (n first); then,
 *             run_device only, alignment in argument order. */
#ifndef IQDEMOD_FSK_H
#define IQDEMOD_FSK_H

#include "iqdemod.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IQD_FSK_ABI_VERSION 1

#define IQD_FSK_NRZI 1u   /* iqd_fsk_config.flags: a 0 bit is a change of tone */

typedef struct iqd_fsk iqd_fsk_t;

typedef struct iqd_fsk_config {
    uint32_t abi_version;        /* IQD_FSK_ABI_VERSION */
    uint32_t n_channels;
    uint32_t corr_len;           /* W */
    uint32_t mark_inc;
    uint32_t space_inc;
    uint32_t baud_inc;           /* b */
    uint32_t loop_shift;
    uint32_t flags;              /* IQD_FSK_NRZI */
    const int16_t *window;       /* [W], or NULL for the rectangular one */
    uint32_t min_len;
    uint32_t max_len;
    uint32_t reserved[4];        /* 0 */
} iqd_fsk_config;                /* 64 bytes */

typedef struct iqd_fsk_frame {
    uint64_t end_sample;
    uint32_t offset;
    uint32_t len;
    uint32_t fcs;
    uint32_t flags;              /* 0 */
} iqd_fsk_frame;                 /* 24 bytes */

typedef struct iqd_fsk_state {
    uint64_t samples;
    uint32_t ph;
    uint32_t prev;
    uint32_t last;
    uint32_t ones;
    uint32_t in_frame;
    uint32_t nbits;
    uint32_t bad_fcs;
    uint32_t frames_total;
} iqd_fsk_state;                 /* 40 bytes */

int iqd_fsk_create(iqd_t *e, const iqd_fsk_config *cfg, iqd_fsk_t **out);
void iqd_fsk_destroy(iqd_fsk_t *t);
int iqd_fsk_reset(iqd_fsk_t *t);
size_t iqd_fsk_max_frames(const iqd_fsk_t *t, size_t n);
size_t iqd_fsk_max_bit_words(const iqd_fsk_t *t, size_t n);
size_t iqd_fsk_max_bytes(const iqd_fsk_t *t, size_t n);
int iqd_fsk_run_device(iqd_t *e, iqd_fsk_t *t, const int16_t *pcm_dev, size_t row_stride, const uint32_t *count_dev, size_t n,
                       uint32_t *n_bits_dev, uint32_t *bits_dev, uint32_t *n_frames_dev, iqd_fsk_frame *frames_dev, uint8_t *bytes_dev);
int iqd_fsk_run(iqd_t *e, iqd_fsk_t *t, const int16_t *pcm, size_t row_stride, const uint32_t *count, size_t n, uint32_t *n_bits,
                uint32_t *bits, uint32_t *n_frames, iqd_fsk_frame *frames, uint8_t *bytes);
int iqd_fsk_get_state(iqd_fsk_t *t, uint32_t channel, iqd_fsk_state *state);

/* host only, no GPU */
int iqd_fsk_phase_inc(uint64_t freq_mhz, uint32_t rate_hz, uint32_t *d);
int iqd_fsk_afsk1200(uint32_t rate_hz, iqd_fsk_config *cfg);

#ifdef __cplusplus
}
#endif
#endif
