"""numpy int64 model of the wideband channelizer's integer spec (include/iqdemod.h: iqd_channelizer_*).

Per channel, plain np.convolve on integer arrays; the GPU's bytes must equal these exactly.  The phasor table is passed
in (the library's own, capi.channelizer_phasor_table()) so that no test depends on two libms agreeing."""
import numpy as np


def phasor_formula():
    i = np.arange(4096)
    return np.stack([np.rint(32767 * np.cos(2 * np.pi * i / 4096)),
                     np.rint(32767 * np.sin(2 * np.pi * i / 4096))], axis=1).astype(np.int16)


def channel_taps(h, inc, P):
    """(gr, gi) int64: i_k = (k d mod 2^32) >> 20, g = (h P + 2^14) >> 15."""
    h = np.asarray(h, np.int64)
    idx = ((np.arange(len(h), dtype=np.uint64) * np.uint64(inc)) & np.uint64(0xffffffff)) >> np.uint64(20)
    idx = idx.astype(np.int64)
    P = np.asarray(P, np.int64)
    return (h * P[idx, 0] + (1 << 14)) >> 15, (h * P[idx, 1] + (1 << 14)) >> 15


def channel(wide_row, h, M, inc, shift, P, m_range=None, stage_a=False):
    """One channel's output bytes (interleaved I, Q offset binary) for the whole stream wide_row (uint8, from sample 0),
    outputs m in m_range (default: all).  stage_a=True returns the int16 stage a = (ar, ai) instead."""
    u = np.asarray(wide_row, np.int64)
    xr, xi = u[0::2] - 128, u[1::2] - 128
    n_out = len(xr) // M
    m0, m1 = (0, n_out) if m_range is None else m_range
    K = len(h)
    lo = max(0, m0 * M + M - 1 - (K - 1))           # the samples these outputs reach
    hi = m1 * M
    xr, xi = xr[lo:hi], xi[lo:hi]
    gr, gi = channel_taps(h, inc, P)
    n = np.arange(m0, m1, dtype=np.int64) * M + M - 1
    at = n - lo                                     # index into the full convolution of the slice
    Ar = (np.convolve(gr, xr) - np.convolve(gi, xi))[at]
    Ai = (np.convolve(gr, xi) + np.convolve(gi, xr))[at]
    ar = np.clip((Ar + 128) >> 8, -32768, 32767)
    ai = np.clip((Ai + 128) >> 8, -32768, 32767)
    if stage_a:
        return ar, ai
    idx = ((n.astype(np.uint64) * np.uint64(inc)) & np.uint64(0xffffffff)) >> np.uint64(20)
    c = np.asarray(P, np.int64)[idx.astype(np.int64), 0]
    s = np.asarray(P, np.int64)[idx.astype(np.int64), 1]
    rr, ri = ar * c + ai * s, ai * c - ar * s
    L = int(shift)
    yr = np.clip((rr + (1 << (21 - L))) >> (22 - L), -128, 127)
    yi = np.clip((ri + (1 << (21 - L))) >> (22 - L), -128, 127)
    out = np.empty(2 * len(n), np.uint8)
    out[0::2] = (yr + 128).astype(np.uint8)
    out[1::2] = (yi + 128).astype(np.uint8)
    return out


def channelize(wide, h, M, sources, incs, shifts, P):
    """All channels: wide [n_sources, bytes] -> [n_ch, bytes / M]."""
    wide = np.asarray(wide).reshape(-1, np.asarray(wide).shape[-1])
    return np.stack([channel(wide[s], h, M, d, L, P) for s, d, L in zip(sources, incs, shifts)])
