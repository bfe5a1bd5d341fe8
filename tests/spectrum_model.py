"""The numpy model of the band spectrum (include/iqdemod.h: "Band spectrum"), in int64, with switchable defects for the
mutation proof of the GPU test's inputs (tests/test_spectrum_host.py).  It takes the window and the phasor table as arrays
and asserts the spec's bounds as it goes.  Nothing here touches a GPU.

The bin sums are formed with a float64 matrix product and converted: every product is below 2^22 and every partial sum
below 2^34, far inside float64's 2^53 integers, so the result is the exact integer sum (and BLAS makes the proof quick)."""
import numpy as np

N_SET = (64, 128, 256, 512, 1024, 2048)

DEFECTS = [
    "no_shift",        # 1  bins not shifted (q = k')
    "conjugate",       # 2  conjugate (mirrored band)
    "iq_swap",         # 3  I and Q exchanged
    "coef_trunc",      # 4  coefficient rounding without the 2^14
    "a_trunc",         # 5  stage a truncating
    "a_round_low",     # 6  stage a rounding with 2^15 - 1
    "hi_wrap",         # 7  hi plane wrapped to int8 without the |v| bound: hi = 128 becomes -128
    "lo_unsigned",     # 8  lo plane read unsigned
    "sum_wrap",        # 9  block sum wrapping at 2^32
    "div_call",        # 10 division by the call's frames instead of F
    "boundary_late",   # 11 block boundary one frame late
    "drop_last",       # 12 last frame of a block dropped
    "source_0",        # 13 every source reads source 0
    "flip",            # 14 U8 not flipped / S8 flipped
    "window_reversed", # 15 window index reversed
]
COEF_DEFECTS = {"no_shift", "conjugate", "coef_trunc", "hi_wrap", "lo_unsigned", "window_reversed"}
INPUT_DEFECTS = {"iq_swap", "source_0", "flip"}


def check_window(w, N):
    w = np.asarray(w, np.int64)
    assert N in N_SET and w.shape == (N,)
    assert np.abs(w).max() <= 32639 and 256 * int(np.abs(w).sum()) <= 2 ** 31 - 256
    return w


def default_window(N, P):
    """w[n] = (32767 - Pc[(2 n + 1) (2048 / N)]) >> sh, sh the smallest value >= 2 with 256 sum w <= 2^31 - 256"""
    Pc = np.asarray(P, np.int64).reshape(4096, 2)[:, 0]
    n = np.arange(N)
    sh = 2
    while True:
        w = (32767 - Pc[(2 * n + 1) * (2048 // N)]) >> sh
        if 256 * int(w.sum()) <= 2 ** 31 - 256:
            return w.astype(np.int16), sh
        sh += 1


def full_scale(w):
    c0 = (32767 * np.asarray(w, np.int64) + 2 ** 14) >> 15
    return int((127 * int(c0.sum()) + 2 ** 15) >> 16) ** 2


def coefficients(w, P, N, defect=None, bounds=True):
    """c, s [N bins, N samples] int64"""
    w = check_window(w, N) if bounds else np.asarray(w, np.int64)
    P = np.asarray(P, np.int64).reshape(4096, 2)
    if defect == "window_reversed":
        w = w[::-1]
    k = np.arange(N)[:, None]
    n = np.arange(N)[None, :]
    q = k if defect == "no_shift" else k - N // 2
    i = ((q * n) % N) * (4096 // N)                 # numpy's % is non-negative for a positive modulus
    rnd = 0 if defect == "coef_trunc" else 2 ** 14
    c = (w[None, :] * P[i, 0] + rnd) >> 15
    s = (w[None, :] * P[i, 1] + rnd) >> 15
    if defect == "conjugate":
        s = -s
    if bounds:
        assert max(np.abs(c).max(), np.abs(s).max()) <= 32639
    return c, s


def planes(v, defect=None, bounds=True):
    """a row value as the kernel's operand planes read it back: hi = (v + 128) >> 8, lo = v - 256 hi"""
    hi = (v + 128) >> 8
    lo = v - 256 * hi
    if bounds and defect is None:
        assert hi.min() >= -128 and hi.max() <= 127 and lo.min() >= -128 and lo.max() <= 127
    if defect == "hi_wrap":
        hi = ((hi + 128) & 0xff) - 128
    if defect == "lo_unsigned":
        lo = lo & 0xff
    return 256 * hi + lo


def samples(wide, fmt, N, defect=None):
    """[n_sources, bytes] of the format's dtype -> xr, xi [n_sources, frames, N] int64"""
    wide = np.asarray(wide)
    assert wide.ndim == 2 and wide.dtype == (np.uint8 if fmt == "u8" else np.int8) and wide.shape[1] % (2 * N) == 0
    b = wide.view(np.uint8)
    if (fmt == "u8") != (defect == "flip"):
        b = b ^ 0x80
    x = b.view(np.int8).astype(np.int64).reshape(wide.shape[0], -1, N, 2)
    if defect == "source_0":
        x = np.broadcast_to(x[:1], x.shape)
    xr, xi = x[..., 0], x[..., 1]
    return (xi, xr) if defect == "iq_swap" else (xr, xi)


def bin_sums(c, s, xr, xi, defect=None, bounds=True):
    """Ar, Ai [n_sources, frames, N bins] int64, through the operand rows (c, s, ...) and (-s, c, ...)"""
    cr, sr = planes(c, defect, bounds), planes(s, defect, bounds)
    ci, nsi = cr, planes(-s, defect, bounds)
    f = np.float64
    Ar = xr.astype(f) @ cr.T.astype(f) + xi.astype(f) @ sr.T.astype(f)
    Ai = xi.astype(f) @ ci.T.astype(f) + xr.astype(f) @ nsi.T.astype(f)
    Ar, Ai = Ar.astype(np.int64), Ai.astype(np.int64)
    if bounds and defect is None:
        assert max(np.abs(Ar).max(), np.abs(Ai).max()) < 2 ** 31
    return Ar, Ai


def frame_power(Ar, Ai, defect=None):
    rnd = {"a_trunc": 0, "a_round_low": 2 ** 15 - 1}.get(defect, 2 ** 15)
    ar, ai = (Ar + rnd) >> 16, (Ai + rnd) >> 16
    if defect is None:
        assert max(np.abs(ar).max(), np.abs(ai).max()) <= 23172
    p = ar * ar + ai * ai
    if defect is None:
        assert p.max() < 2 ** 31
    return p


def reduce(p, F, defect=None):
    """p [n_sources, frames, N] -> power [n_sources, n_blocks, N] uint32"""
    S, T, N = p.shape
    assert 1 <= F <= 2 ** 24 and T > 0 and T % F == 0
    nb = T // F
    out = np.zeros((S, nb, N), np.int64)
    for b in range(nb):
        lo, hi = b * F, (b + 1) * F
        if defect == "boundary_late":
            lo, hi = lo + 1, min(hi + 1, T)
        if defect == "drop_last":
            hi -= 1
        tot = p[:, lo:hi].sum(axis=1)
        if defect == "sum_wrap":
            tot = tot & 0xffffffff
        out[:, b] = tot // (T if defect == "div_call" else F)
    assert out.max() < 2 ** 32
    return out.astype(np.uint32)


class Model:
    """One case's model with the intermediate results shared between the defects that do not touch them."""

    def __init__(self, wide, fmt, N, F, w, P):
        self.wide, self.fmt, self.N, self.F, self.w, self.P = wide, fmt, N, F, w, P
        self._cs, self._x, self._A = {}, {}, {}

    def sums(self, defect=None):
        dc = defect if defect in COEF_DEFECTS else None
        dx = defect if defect in INPUT_DEFECTS else None
        if (dc, dx) not in self._A:
            if dc not in self._cs:
                self._cs[dc] = coefficients(self.w, self.P, self.N, dc)
            if dx not in self._x:
                self._x[dx] = samples(self.wide, self.fmt, self.N, dx)
            self._A[(dc, dx)] = bin_sums(*self._cs[dc], *self._x[dx], dc)
        return self._A[(dc, dx)]

    def power(self, defect=None):
        assert defect is None or defect in DEFECTS
        return reduce(frame_power(*self.sums(defect), defect), self.F, defect)


def spectrum(wide, fmt, N, F, w, P, defect=None):
    """power[n_sources][n_blocks][N] uint32 of the spec; w None: the default window"""
    if w is None:
        w = default_window(N, P)[0]
    return Model(wide, fmt, N, F, w, P).power(defect)


def fft_power(wide, fmt, N, F, w):
    """The same windowed frames through numpy's float64 FFT, fftshifted and scaled by 32767 / 32768 / 65536: float64
    [n_sources, n_blocks, N].  Independent of everything above but the sample decoding."""
    xr, xi = samples(wide, fmt, N)
    X = np.fft.fftshift(np.fft.fft((xr + 1j * xi) * np.asarray(w, np.float64), axis=-1), axes=-1)
    p = np.abs(X * (32767.0 / 32768.0 / 65536.0)) ** 2
    return p.reshape(p.shape[0], -1, F, N).mean(axis=2)
