"""numpy / Python-integer model of the PCM packet decoder, written from the text of include/iqdemod_fsk.h (not from the
kernel): the oracle of tests/test_gpu_fsk*.py, with switchable defects for the mutation proof of tests/test_fsk_host.py.

Model(n_channels, phasor, corr_len, mark_inc, space_inc, baud_inc, loop_shift, flags, window=None, min_len, max_len, defect=None)
  .run(pcm [C, stride] int16, n, count=None) -> (n_bits [C] u32, bits [C, Bw] u32, n_frames [C] u32, frames [C, F] FRAME,
                                                 bytes [C, Bc] u8)
  .reset(), .state(ch) -> dict(samples, ph, prev, last, ones, in_frame, nbits, bad_fcs, frames_total)
phasor is the library's table, [4096, 2] int16 (capi.channelizer_phasor_table()).  The correlator sums are int64 (< 2^28);
soft is formed in Python integers."""
import numpy as np

FRAME = np.dtype([("end_sample", "<u8"), ("offset", "<u4"), ("len", "<u4"), ("fcs", "<u4"), ("flags", "<u4")])
NRZI = 1
MAX_WINDOW = 32512

# each a plausible error of a kernel or of its host code
DEFECTS = {
    "soft_ge": "d = 1 for soft >= 0: silence and a tie decide 1",
    "phase_from_stream": "the coefficients' phase counted from the stream's sample index instead of the window's first sample",
    "coef_no_round": "the coefficients without the 2^22 rounding term",
    "nudge_after_inc": "the clock's nudge applied after the increment (and its carry) instead of before",
    "nudge_reversed": "the nudge's comparison reversed: ph >= 2^31 advances",
    "nrzi_polarity": "NRZI with a change read as 1",
    "stuff_after_six": "the stuffed zero taken after six ones instead of five (a flag is then never seen)",
    "nbits_kept": "nbits not cleared at a flag",
    "lb_minus_8": "Lb = nbits - 8",
    "msb_first": "bytes assembled MSB first",
    "crc_init_0": "the CRC started at 0",
    "fcs_swapped": "the FCS compared as byte[-2] << 8 | byte[-1]",
    "history_dropped": "the correlators' W - 1 carried samples taken as zeros at every call",
    "max_len_off": "a frame of exactly max_len bytes overflows",
    "end_sample_off": "end_sample one too large",
    "count_ignored": "count ignored: every row taken as n samples",
}


def phase_inc(freq_mhz, rate_hz):
    return (freq_mhz * 2 ** 32 + 500 * rate_hz) // (1000 * rate_hz)


def afsk1200(rate_hz):
    return dict(corr_len=8, mark_inc=phase_inc(1200000, rate_hz), space_inc=phase_inc(2200000, rate_hz),
                baud_inc=phase_inc(1200000, rate_hz), loop_shift=3, flags=NRZI, min_len=17, max_len=512)


def crc16_x25(data, init=0xffff):
    crc = init
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    return crc ^ 0xffff


def coefficients(window, inc, phasor, first=None, rounding=1 << 22):
    """[2, W] int64 (c, s) with the phase counted from the window's first sample; `first` [m]: the stream index of each
    window's first sample instead -> [m, 2, W]"""
    W = len(window)
    k = np.arange(W, dtype=np.int64)
    if first is not None:
        k = np.asarray(first, np.int64)[:, None] + k[None, :]
    i = ((k.astype(np.uint64) * np.uint64(int(inc))) & np.uint64(0xffffffff)) >> np.uint64(20)
    w = np.asarray(window, np.int64)
    out = np.stack([(w * phasor[i.astype(np.int64), h].astype(np.int64) + rounding) >> 23 for h in range(2)], axis=-2)
    return out


class Model:
    def __init__(self, n_channels, phasor, corr_len, mark_inc, space_inc, baud_inc, loop_shift, flags=NRZI, window=None, min_len=17,
                 max_len=512, defect=None):
        assert defect is None or defect in DEFECTS
        self.C, self.W, self.defect, self.phasor = int(n_channels), int(corr_len), defect, phasor
        self.mark_inc, self.space_inc, self.b, self.shift = int(mark_inc), int(space_inc), int(baud_inc), int(loop_shift)
        self.nrzi, self.min_len, self.max_len = bool(flags & NRZI), int(min_len), int(max_len)
        assert 2 <= self.W <= 64 and 2 ** 20 <= self.b < 2 ** 31 and 1 <= self.shift <= 8 and not flags & ~NRZI
        assert 3 <= self.min_len <= self.max_len <= 1024
        self.window = np.full(self.W, MAX_WINDOW, np.int64) if window is None else np.asarray(window, np.int64)
        assert len(self.window) == self.W and np.abs(self.window).max() <= MAX_WINDOW
        rounding = 0 if defect == "coef_no_round" else 1 << 22
        self.rounding = rounding
        self.coef = np.concatenate([coefficients(self.window, d, phasor, rounding=rounding) for d in (self.mark_inc, self.space_inc)])
        assert np.abs(self.coef).max() <= 127
        self.reset()

    def reset(self):
        self.hist = [np.zeros(self.W - 1, np.int64) for _ in range(self.C)]
        self.st = [dict(samples=0, ph=0, prev=0, last=0, ones=0, in_frame=0, nbits=0, bad_fcs=0, frames_total=0) for _ in range(self.C)]
        self.buf = [[] for _ in range(self.C)]

    def state(self, ch):
        return dict(self.st[ch])

    # the header's sizes
    def maxbits(self, n):
        return (n * (self.b + (self.b >> self.shift))) // 2 ** 32 + 1 if n else 0

    def max_frames(self, n):
        return self.maxbits(n) // (8 * self.min_len + 8) + 1 if n else 0

    def max_bit_words(self, n):
        return (self.maxbits(n) + 31) // 32

    def max_bytes(self, n):
        return (self.max_len + self.maxbits(n) // 8 + 15) // 16 * 16 if n else 0

    def decisions(self, c, x):
        """d[j] of the call's samples x of channel c; moves the carried samples"""
        W = self.W
        hist = np.zeros(W - 1, np.int64) if self.defect == "history_dropped" else self.hist[c]
        s = np.concatenate([hist, x])
        self.hist[c] = np.concatenate([self.hist[c], x])[len(x):]
        if len(x) == 0:
            return []
        win = np.lib.stride_tricks.sliding_window_view(s, W)            # [m, W]: window j is x[j - W + 1 .. j]
        if self.defect == "phase_from_stream":
            first = self.st[c]["samples"] + np.arange(len(x), dtype=np.int64) - W + 1
            coef = np.concatenate([coefficients(self.window, d, self.phasor, first=first, rounding=self.rounding)
                                   for d in (self.mark_inc, self.space_inc)], axis=1)   # [m, 4, W]
            acc = np.einsum("mhk,mk->mh", coef, win)
        else:
            acc = win @ self.coef.T                                      # [m, 4] Mr, Mi, Sr, Si
        assert np.abs(acc).max() < 2 ** 28
        out = []
        for mr, mi, sr, si in acc.tolist():                              # Python integers
            soft = mr * mr + mi * mi - sr * sr - si * si
            assert abs(soft) < 2 ** 57
            out.append(int(soft >= 0 if self.defect == "soft_ge" else soft > 0))
        return out

    def _append(self, c, bit):
        st, buf = self.st[c], self.buf[c]
        del buf[st["nbits"]:]
        buf.append(bit)
        st["nbits"] += 1
        limit = 8 * self.max_len + 7 - (8 if self.defect == "max_len_off" else 0)
        if st["nbits"] > limit:
            st["in_frame"] = 0

    def _close(self, c, j, out):
        st, buf, d = self.st[c], self.buf[c], self.defect
        Lb = st["nbits"] - (8 if d == "lb_minus_8" else 7)
        if Lb < 8 * self.min_len or Lb % 8:
            return
        data = []
        for i in range(Lb // 8):
            bits = buf[8 * i:8 * i + 8]
            data.append(sum(b << (7 - k if d == "msb_first" else k) for k, b in enumerate(bits)))
        crc = crc16_x25(data[:-2], 0 if d == "crc_init_0" else 0xffff)
        fcs = data[-2] << 8 | data[-1] if d == "fcs_swapped" else data[-2] | data[-1] << 8
        if crc == fcs:
            out.append((st["samples"] + j + (1 if d == "end_sample_off" else 0), bytes(data[:-2]), fcs))
            st["frames_total"] = min(st["frames_total"] + 1, 2 ** 32 - 1)
        else:
            st["bad_fcs"] = min(st["bad_fcs"] + 1, 2 ** 32 - 1)

    def _bit(self, c, bit, j, out):
        st, d = self.st[c], self.defect
        stuffed = 6 if d == "stuff_after_six" else 5
        if bit:
            st["ones"] = min(st["ones"] + 1, 7)
            if st["ones"] == 7:
                st["in_frame"] = 0
            elif st["in_frame"]:
                self._append(c, 1)
        else:
            o, st["ones"] = st["ones"], 0
            if o == stuffed:
                pass
            elif o == 6:
                if st["in_frame"]:
                    self._close(c, j, out)
                st["in_frame"] = 1
                if d != "nbits_kept":
                    st["nbits"] = 0
            elif st["in_frame"]:
                self._append(c, 0)

    def walk(self, c, dec):
        """the call's decisions of channel c -> (bits after NRZI, [(end_sample, payload, fcs)])"""
        st, d, b = self.st[c], self.defect, self.b
        g = b >> self.shift
        bits, frames = [], []
        ph, prev, half = st["ph"], st["prev"], 2 ** 31
        late, flip = d == "nudge_after_inc", d == "nudge_reversed"
        for j, dj in enumerate(dec):
            changed = dj != prev
            prev = dj
            if changed and not late:
                ph = (ph + (g if (ph < half) != flip else -g)) % 2 ** 32
            ph += b
            carry = ph >= 2 ** 32
            ph %= 2 ** 32
            if changed and late:
                ph = (ph + (g if (ph < half) != flip else -g)) % 2 ** 32
            if not carry:
                continue
            if self.nrzi:
                bit = int(dj == st["last"])
                if d == "nrzi_polarity":
                    bit ^= 1
                st["last"] = dj
            else:
                bit = dj
            bits.append(bit)
            self._bit(c, bit, j, frames)
        st["ph"], st["prev"] = ph, prev
        st["samples"] += len(dec)
        return bits, frames

    def run(self, pcm, n, count=None):
        pcm = np.asarray(pcm, np.int16).reshape(self.C, -1)
        n = int(n)
        assert 0 <= n <= pcm.shape[1]
        F, Bw, Bc = self.max_frames(n), self.max_bit_words(n), self.max_bytes(n)
        nb, nf = np.zeros(self.C, np.uint32), np.zeros(self.C, np.uint32)
        bitw, frames, data = np.zeros((self.C, Bw), np.uint32), np.zeros((self.C, F), FRAME), np.zeros((self.C, Bc), np.uint8)
        for c in range(self.C):
            m = n if count is None or self.defect == "count_ignored" else min(int(count[c]), n)
            bits, found = self.walk(c, self.decisions(c, pcm[c, :m].astype(np.int64)))
            assert len(bits) <= self.maxbits(n) and len(found) <= F
            nb[c], nf[c] = len(bits), len(found)
            for i, bit in enumerate(bits):
                bitw[c, i // 32] |= np.uint32(bit << (i % 32))
            off = 0
            for k, (end, payload, fcs) in enumerate(found):
                frames[c, k] = (end, off, len(payload), fcs, 0)
                data[c, off:off + len(payload)] = np.frombuffer(payload, np.uint8)
                off += len(payload)
            assert off <= Bc
        return nb, bitw, nf, frames, data


# ---- the transmit side, for tests: frames -> line bits -> audio ----

def hdlc_bits(payloads, lead_flags=2, between_flags=1, tail_flags=2, bad_fcs=()):
    """the bit stream (before NRZI) of frames between flags: each payload with its FCS (wrong for the indices in bad_fcs),
    bit-stuffed"""
    flag = [0, 1, 1, 1, 1, 1, 1, 0]
    out = flag * lead_flags
    for k, p in enumerate(payloads):
        crc = crc16_x25(p) ^ (0x0101 if k in bad_fcs else 0)
        ones = 0
        for byte in list(p) + [crc & 255, crc >> 8]:
            for i in range(8):
                bit = byte >> i & 1
                out.append(bit)
                ones = ones + 1 if bit else 0
                if ones == 5:
                    out.append(0)
                    ones = 0
        out += flag * (between_flags if k + 1 < len(payloads) else tail_flags)
    return out


def nrzi_levels(bits, level=1):
    """a 0 bit is a change of level, a 1 bit none; the level before the first bit is `level`"""
    out = []
    for b in bits:
        if not b:
            level ^= 1
        out.append(level)
    return out


def afsk(levels, phasor, mark_inc, space_inc, baud_inc, amp=8000, n=None):
    """continuous-phase audio of a level per bit (1 = mark) from the table's cosines: integers only.  A bit lasts until the
    baud accumulator carries; n: stop after n samples (default: the end of the last bit)."""
    out, ph, clock, i = [], 0, 0, 0
    while i < len(levels) and (n is None or len(out) < n):
        out.append((amp * int(phasor[ph >> 20, 0])) >> 15)
        ph = (ph + (mark_inc if levels[i] else space_inc)) % 2 ** 32
        clock += baud_inc
        if clock >= 2 ** 32:
            clock -= 2 ** 32
            i += 1
    return np.array(out, np.int64)
