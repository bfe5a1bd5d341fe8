"""The inputs of the band spectrum's GPU test (tests/test_gpu_spectrum.py), built here so that the CPU tier can hold the
very same inputs to the mutation proof (tests/test_spectrum_host.py).  Everything is seeded; nothing here touches a GPU.
A case is one Spectrum object (N, window, format, sources) and one call of `blocks` blocks of F frames.

The kernel takes a block's frames 64 at a time (iqd_spectrum.h: SPC_CHUNK) and the rest as 1 .. 4 tiles of 16 frames, so
F = 104 is a whole chunk and three tiles, F = 60 four tiles with a ragged last one, F = 32 two, F = 1, 2, 3 one."""
import numpy as np

from tests import spectrum_model as sm

CHUNK = 64


def tone(N, frames, cycles_per_frame, amp=127.0):
    """a full-scale complex tone, `cycles_per_frame` cycles per N samples (a bin centre when an integer), as int8 rails"""
    n = np.arange(N * frames)
    z = amp * np.exp(2j * np.pi * cycles_per_frame * n / N)
    x = np.empty(2 * N * frames, np.int8)
    x[0::2] = np.rint(z.real).astype(np.int8)
    x[1::2] = np.rint(z.imag).astype(np.int8)
    return x


class Case:
    def __init__(self, name, N, F, blocks, fmt, window, rows, tones=None):
        """rows: [n_sources, 2 N F blocks] int8 - the signal; a u8 case stores it offset binary"""
        rows = np.ascontiguousarray(rows, np.int8)
        assert rows.ndim == 2 and rows.shape[1] == 2 * N * F * blocks
        self.name, self.N, self.F, self.blocks, self.fmt, self.n_src = name, N, F, blocks, fmt, rows.shape[0]
        self.window = None if window is None else np.ascontiguousarray(window, np.int16)   # None: the library's default
        self.wide = (rows.view(np.uint8) ^ 0x80) if fmt == "u8" else rows
        self.tones = tones            # per source: the bin the strongest line must fall on

    def w(self, P):
        return sm.default_window(self.N, P)[0] if self.window is None else self.window

    def __repr__(self):
        return self.name


NAMES = ["N64-F1-random", "N64-F32-random", "N64-F104-neg", "N128-F3-ramp-s8", "N64-F60-s8", "N1024-quiet", "N1024-const-F32",
         "N1024-tones", "N1024-rails-8191-s8", "N64-rails-32639", "N64-half-point", "N2048-F2-s8"]


def cases(P):
    """P: the phasor table, [4096, 2] int16 (capi.channelizer_phasor_table())"""
    def rnd(seed, n_src, nbytes):
        return np.random.default_rng(seed).integers(-128, 128, (n_src, nbytes)).astype(np.int8)

    out = [
        # a frame is two MFMA K steps; one frame per block
        Case("N64-F1-random", 64, 1, 3, "u8", None, rnd(401, 3, 2 * 64 * 3)),
        Case("N64-F32-random", 64, 32, 3, "u8", None, rnd(402, 1, 2 * 64 * 32 * 3)),
    ]
    # a window with negative entries (a flat-top-like shape: 5 cycles of a cosine on a pedestal), asymmetric by a slope;
    # F = 104: more frames than a wave takes at once
    n = np.arange(64)
    neg = np.rint(9000 * np.cos(2 * np.pi * 5 * n / 64) + 3000 + 40 * n).astype(np.int16)
    assert neg.min() < 0
    out.append(Case("N64-F104-neg", 64, 104, 2, "u8", neg, rnd(403, 1, 2 * 64 * 104 * 2)))
    ramp = (np.arange(128) * 250 + 100).astype(np.int16)                      # asymmetric
    out.append(Case("N128-F3-ramp-s8", 128, 3, 2, "s8", ramp, rnd(404, 1, 2 * 128 * 3 * 2)))
    out.append(Case("N64-F60-s8", 64, 60, 1, "s8", None, rnd(405, 3, 2 * 64 * 60)))
    # all quiet: U8 0x80, the power is exactly 0
    out.append(Case("N1024-quiet", 1024, 2, 1, "u8", None, np.zeros((1, 2 * 1024 * 2), np.int8)))
    # the constant (255, 128): every frame gives p_fs = 264225025 at bin N / 2, and the block sum 32 p_fs passes 2^32
    const = np.zeros((1, 1024 * 32, 2), np.int8)
    const[..., 0] = 127
    out.append(Case("N1024-const-F32", 1024, 32, 1, "u8", None, const.reshape(1, -1)))
    # full-scale tones: on a bin centre, and between bins at a positive and at a negative offset (the nearer bin is named)
    cyc = [100.0, 200.25, -300.25]
    out.append(Case("N1024-tones", 1024, 2, 1, "u8", None, np.stack([tone(1024, 2, c) for c in cyc]),
                    tones=[512 + 100, 512 + 200, 512 - 300]))
    # sign-matched rails under a rectangular window at the limit of 256 sum |w|: the largest |Ar| (frame 0, bin 700) and
    # |Ai| (frame 1, bin 3) the spec allows
    def rails(N, w, bins):
        fr = np.zeros((len(bins), N, 2), np.int8)
        for f, (k, which) in enumerate(bins):
            c, s = sm.coefficients(w, P, N)
            c, s = c[k], s[k]
            if which == "r":      # Ar = sum c xr + s xi
                fr[f, :, 0] = np.where(c >= 0, 127, -128)
                fr[f, :, 1] = np.where(s >= 0, 127, -128)
            else:                 # Ai = sum c xi - s xr
                fr[f, :, 1] = np.where(c >= 0, 127, -128)
                fr[f, :, 0] = np.where(s >= 0, -128, 127)
        return fr.reshape(1, -1)
    w8191 = np.full(1024, 8191, np.int16)
    out.append(Case("N1024-rails-8191-s8", 1024, 1, 2, "s8", w8191, rails(1024, w8191, [(700, "r"), (3, "i")])))
    w32639 = np.full(64, 32639, np.int16)
    out.append(Case("N64-rails-32639", 64, 2, 1, "u8", w32639, rails(64, w32639, [(41, "r"), (9, "i")])))
    # Planted frames whose Ar lies exactly on stage a's half point.  w = 1024 everywhere makes c = 1024, s = 0 at bin N / 2,
    # so Ar = 1024 sum xr there: 32 samples of +1 give Ar = +2^15 (a = 1, truncated or rounded low: 0), 32 of -1 give
    # Ar = -2^15 (a = 0, truncated: -1).  One frame per block.
    half = np.zeros((1, 2, 64, 2), np.int8)
    half[0, 0, :32, 0] = 1
    half[0, 1, :32, 0] = -1
    out.append(Case("N64-half-point", 64, 1, 2, "u8", np.full(64, 1024, np.int16), half.reshape(1, -1)))
    # the largest operand (32 MiB), the default window's sh = 3
    out.append(Case("N2048-F2-s8", 2048, 2, 2, "s8", None, rnd(406, 1, 2 * 2048 * 2 * 2)))
    assert [c.name for c in out] == NAMES
    return out
