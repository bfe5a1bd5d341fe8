"""numpy / Python-integer model of the PCM tone bank, written from the text of include/iqdemod_tones.h (not from the kernel):
the oracle of tests/test_gpu_tones*.py, with switchable defects for the mutation proof of tests/test_tones_host.py.

Model(n_channels, L, incs, phasor, window=None, min_power=0, ratio_q8=256, energy_q8=0, open=1, hold=0, defect=None)
  .run(pcm [C, stride] int16, n, count=None) -> (n_frames [C] uint32, frames [C, F] FRAME, power [C, F, T] uint64)
  .reset(), .state(ch) -> dict(tone, cand, run, miss, fill)
phasor is the library's table, [4096, 2] int16 (capi.channelizer_phasor_table()).  Sums are int64 (|A| < 2^44, p < 2^57),
the hit's products Python integers."""
import numpy as np

FRAME = np.dtype([("energy", "<u8"), ("p_best", "<u8"), ("p_second", "<u8"), ("best", "<u4"), ("second", "<u4"),
                  ("tone", "<i4"), ("flags", "<u4")])
F_OPENED, F_CLOSED = 1, 2
NONE = 0xffffffff

# each a plausible error of a kernel or of its host code.  (c and s swapped is none of them: p = ar^2 + ai^2 is the same, no
# output can show it.)
DEFECTS = {
    "phase_from_call": "the phase counted from the call's first sample instead of the frame's",
    "carry_dropped": "the open frame's samples lost at a call boundary (the fill kept)",
    "no_round": "ar = A >> 16 without the 2^15",
    "trunc_shift": "a truncating shift (towards zero) for negative A",
    "low_plane_unsigned": "the samples' low byte plane taken as signed without its re-bias",
    "tie_high": "the highest index wins a tie of powers",
    "second_is_best": "second allowed to equal best",
    "ratio_wrap64": "the ratio product wrapped at 64 bits",
    "miss_ge_hold": "closing at miss >= hold instead of miss > hold",
    "switch_loses_open": "a frame that closes does not open (the switch's OPENED lost)",
    "count_ignored": "count ignored: every row taken as n samples",
    "tail_not_zeroed": "records and power rows past k_c left as the previous frame's",
    "reset_keeps_frame": "reset clears the decision state and keeps the open frame",
}


def default_window(L, phasor):
    n = np.arange(L, dtype=np.int64)
    return ((32767 - phasor[((2 * n + 1) * 2048) // L, 0].astype(np.int64)) >> 2).astype(np.int16)


def phase_inc(freq_mhz, rate_hz):
    return (freq_mhz * 2 ** 32 + 500 * rate_hz) // (1000 * rate_hz)


def coefficients(L, incs, window, phasor):
    """[T, 2, L] int64: c_t[n], s_t[n]"""
    n = np.arange(L, dtype=np.uint64)
    out = np.zeros((len(incs), 2, L), np.int64)
    w = np.asarray(window, np.int64)
    for t, d in enumerate(incs):
        i = (((n * np.uint64(int(d))) & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.int64)
        for h in range(2):
            out[t, h] = (w * phasor[i, h].astype(np.int64) + (1 << 14)) >> 15
    return out


class Model:
    def __init__(self, n_channels, L, incs, phasor, window=None, min_power=0, ratio_q8=256, energy_q8=0, open=1, hold=0, defect=None):
        assert defect is None or defect in DEFECTS
        self.C, self.L, self.T, self.defect = int(n_channels), int(L), len(incs), defect
        self.incs = [int(d) for d in incs]
        self.phasor = phasor
        self.window = default_window(L, phasor) if window is None else np.asarray(window, np.int16)
        self.coef = coefficients(L, self.incs, self.window, phasor)
        self.min_power, self.ratio_q8, self.energy_q8, self.open, self.hold = int(min_power), int(ratio_q8), int(energy_q8), int(open), int(hold)
        self.reset(first=True)

    def reset(self, first=False):
        if first or self.defect != "reset_keeps_frame":
            self.frame = [np.zeros(0, np.int64) for _ in range(self.C)]
        self.dec = [dict(tone=-1, cand=-1, run=0, miss=0) for _ in range(self.C)]

    def state(self, ch):
        return dict(self.dec[ch], fill=len(self.frame[ch]))

    def max_frames(self, n):
        return (n + self.L - 1) // self.L

    # one frame's powers and energy
    def _frame(self, x, first_in_call):
        L, d = self.L, self.defect
        coef = self.coef
        if d == "phase_from_call" and first_in_call:       # the frame began `first_in_call` samples before the call did
            coef = coefficients_shifted(L, self.incs, self.window, self.phasor, first_in_call)
        xx = x
        if d == "low_plane_unsigned":                       # x = 256 hi + lo with lo read as a signed byte
            lo = x & 255
            xx = (x - lo) + np.where(lo >= 128, lo - 256, lo)
        A = coef @ xx                                       # [T, 2]
        if d == "no_round":
            a = A >> 16
        elif d == "trunc_shift":
            a = np.where(A + 32768 >= 0, (A + 32768) >> 16, -((-(A + 32768)) >> 16))
        else:
            a = (A + 32768) >> 16
        p = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]
        return p.astype(np.uint64), int(np.sum(x * x))

    def _pick(self, p):
        p = [int(v) for v in p]
        T = len(p)
        high = self.defect == "tie_high"
        order = sorted(range(T), key=lambda t: (-p[t], -t if high else t))
        best = order[0]
        if T == 1:
            return best, NONE, 0
        second = best if self.defect == "second_is_best" else order[1]
        return best, second, p[second]

    def _hit(self, pb, ps, E):
        rhs = self.ratio_q8 * ps
        lhs = 256 * pb
        if self.defect == "ratio_wrap64":
            rhs, lhs = rhs % 2 ** 64, lhs % 2 ** 64
        return pb >= self.min_power and lhs >= rhs and 256 * pb >= self.energy_q8 * E

    def _decide(self, s, f):
        flags = 0
        if f >= 0 and f == s["cand"]:
            s["run"] = min(s["run"] + 1, 2 ** 32 - 1)
        else:
            s["cand"], s["run"] = f, int(f >= 0)
        closed = False
        if s["tone"] >= 0:
            s["miss"] = 0 if f == s["tone"] else s["miss"] + 1
            if s["miss"] >= self.hold if self.defect == "miss_ge_hold" else s["miss"] > self.hold:
                s["tone"], s["miss"], flags, closed = -1, 0, flags | F_CLOSED, True
        if s["tone"] < 0 and s["cand"] >= 0 and s["run"] >= self.open and not (closed and self.defect == "switch_loses_open"):
            s["tone"], s["miss"], flags = s["cand"], 0, flags | F_OPENED
        return flags

    def run(self, pcm, n, count=None):
        pcm = np.asarray(pcm, np.int16).reshape(self.C, -1)
        n, L = int(n), self.L
        assert 0 <= n <= pcm.shape[1]
        F = self.max_frames(n)
        nf = np.zeros(self.C, np.uint32)
        frames = np.zeros((self.C, F), FRAME)
        power = np.zeros((self.C, F, self.T), np.uint64)
        for c in range(self.C):
            m = n if count is None or self.defect == "count_ignored" else min(int(count[c]), n)
            carried = len(self.frame[c])
            held = self.frame[c]
            if self.defect == "carry_dropped":
                held = np.zeros(carried, np.int64)
            s = np.concatenate([held, pcm[c, :m].astype(np.int64)])
            k = len(s) // L
            for j in range(k):
                p, E = self._frame(s[j * L:(j + 1) * L], carried if j == 0 else 0)
                best, second, ps = self._pick(p)
                pb = int(p[best])
                f = best if self._hit(pb, ps, E) else -1
                flags = self._decide(self.dec[c], f)
                frames[c, j] = (E, pb, ps, best, second, self.dec[c]["tone"], flags)
                power[c, j] = p
            if self.defect == "tail_not_zeroed" and 0 < k < F:
                frames[c, k:] = frames[c, k - 1]
                power[c, k:] = power[c, k - 1]
            self.frame[c] = s[k * L:]
            nf[c] = k
        return nf, frames, power


def coefficients_shifted(L, incs, window, phasor, shift):
    """the coefficients with the phase counted from `shift` samples into the frame (the window stays the frame's)"""
    n = (np.arange(L, dtype=np.int64) - shift).astype(np.uint64) & np.uint64(0xffffffff)
    out = np.zeros((len(incs), 2, L), np.int64)
    w = np.asarray(window, np.int64)
    for t, d in enumerate(incs):
        i = (((n * np.uint64(int(d))) & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.int64)
        for h in range(2):
            out[t, h] = (w * phasor[i, h].astype(np.int64) + (1 << 14)) >> 15
    return out
