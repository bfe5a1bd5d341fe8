"""numpy int64 model of the channelizer on signed captures (include/iqdemod.h: "Signed captures"; IQD_WIDE_S8, IQD_WIDE_S16),
built on tests/chan_model.py's taps and phasor; every sum is an int64 (|A| < 2^40).  The GPU's bytes must equal these exactly.

`defect` switches on one fault a wrong kernel could plausibly have (DEFECTS); tests/test_chan_fmt_host.py proves that the
inputs of tests/chan_fmt_cases.py expose each of them."""
import numpy as np

from tests import chan_model as cm

DTYPE = {"s8": np.dtype(np.int8), "s16": np.dtype("<i2")}
RAIL_BYTES = {"s8": 1, "s16": 2}

DEFECTS = {
    "lo_signed": "S16: the low byte taken as signed (x = 256 hi + int8(lo))",
    "no_g": "S16: the 128 G term dropped (A = 256 H + Lo')",
    "g_sign": "S16: the 128 G term with gi's sign wrong on the real rail (G_r = sum gr + sum gi)",
    "big_endian": "S16: the bytes of a sample swapped",
    "round_m1": "stage a rounds with 2^15 - 1 (S8: 127)",
    "trunc": "stage a shifts without rounding",
    "wrap32": "S16: 256 H + Lo formed in wrapping int32",
    "s8_flip": "S8: flipped like U8 (taken as offset binary)",
    "hist_lo0": "S16: zero history staged as lo' = 0, so that it reads as +128 on both rails",
    "hist_short": "the history carries only the last Kp B bytes (Kp / 2 samples) across calls; older ones read as 0",
    "iq_swap": "the I and Q planes exchanged",
}
S16_ONLY = {"lo_signed", "no_g", "g_sign", "big_endian", "wrap32", "hist_lo0"}
S8_ONLY = {"s8_flip"}


def applies(defect, fmt):
    return defect not in (S8_ONLY if fmt == "s16" else S16_ONLY)


def samples(wide_row, fmt, defect=None):
    """(xr, xi) int64 of one source's interleaved rails"""
    w = np.asarray(wide_row)
    assert w.dtype == DTYPE[fmt], (w.dtype, fmt)
    if fmt == "s16":
        u = w.astype(np.int64) & 0xffff
        hi, lo = u >> 8, u & 0xff
        if defect == "big_endian":
            hi, lo = lo, hi
        hi = hi - ((hi & 0x80) << 1)                          # signed
        if defect == "lo_signed":
            lo = lo - ((lo & 0x80) << 1)
        x = 256 * hi + lo
    else:
        x = w.astype(np.int64)
        if defect == "s8_flip":
            x = ((x & 0xff) ^ 0x80) - (((x & 0xff) ^ 0x80) & 0x80) * 2
    xr, xi = x[0::2], x[1::2]
    return (xi, xr) if defect == "iq_swap" else (xr, xi)


def channelize(wide, fmt, h, M, sources, incs, shifts, P, defect=None, calls=None, stage_a=False, m_range=None,
               stale_g=None):
    """All channels: wide [n_sources, 2 samples] of the format's dtype, the whole stream from sample 0 -> [n_ch, 2 n_out]
    uint8.  calls: the samples per call, in order (default: one call); only hist_short depends on it.  m_range = (m0, m1):
    outputs m0 <= m < m1 of that stream only (default: all of them).  stale_g: per channel the increment whose coefficient
    sums G enter S16's 128 G term instead of the channel's own - what a retune gives whose new sums never reach the kernel."""
    wide = np.asarray(wide)
    wide = wide.reshape(-1, wide.shape[-1])
    h = np.asarray(h, np.int64)
    K, kp = len(h), (len(h) + 31) // 32 * 32
    n_samp = wide.shape[1] // 2
    n_out = n_samp // M
    m0, m1 = (0, n_out) if m_range is None else m_range
    n = np.arange(m0, m1, dtype=np.int64) * M + M - 1
    n_out = len(n)
    shift16, half = (16, 1 << 15) if fmt == "s16" else (8, 128)
    if defect == "round_m1":
        half -= 1
    if defect == "trunc":
        half = 0
    starts = np.cumsum([0] + list(calls if calls is not None else [n_samp]))[:-1]
    call_of = np.searchsorted(starts, n, side="right") - 1    # the call that emits output m
    out = np.zeros((len(sources), n_out if stage_a else 2 * n_out), np.complex128 if stage_a else np.uint8)
    Pt = np.asarray(P, np.int64)
    for s in sorted(set(int(v) for v in sources)):
        chs = [c for c in range(len(sources)) if int(sources[c]) == s]
        xr, xi = samples(wide[s], fmt, defect)
        pad = 128 if defect == "hist_lo0" and fmt == "s16" else 0
        xr = np.concatenate([np.full(K - 1, pad, np.int64), xr])
        xi = np.concatenate([np.full(K - 1, pad, np.int64), xi])
        # X[m, k] = x[n_m - k]
        Xr = np.lib.stride_tricks.sliding_window_view(xr, K)[n][:, ::-1]
        Xi = np.lib.stride_tricks.sliding_window_view(xi, K)[n][:, ::-1]
        if defect == "hist_short":                            # samples older than kp / 2 before the call's start: 0
            age = n[:, None] - np.arange(K)[None, :]          # the sample index of X[m, k]
            first = starts[call_of][:, None] - kp // 2
            lost = (age < first) & (starts[call_of][:, None] > 0)
            Xr, Xi = np.where(lost, 0, Xr), np.where(lost, 0, Xi)
        g = [cm.channel_taps(h, int(incs[c]), P) for c in chs]
        Gr = np.stack([a for a, _ in g], axis=1)              # [K, n]
        Gi = np.stack([b for _, b in g], axis=1)
        Ar = Xr @ Gr - Xi @ Gi
        Ai = Xi @ Gr + Xr @ Gi
        if fmt == "s16" and stale_g is not None:
            o = [cm.channel_taps(h, int(stale_g[c]), P) for c in chs]
            Or, Oi = np.stack([a for a, _ in o], axis=1).sum(0), np.stack([b for _, b in o], axis=1).sum(0)
            Ar, Ai = Ar + 128 * (Or - Oi - Gr.sum(0) + Gi.sum(0)), Ai + 128 * (Or + Oi - Gr.sum(0) - Gi.sum(0))
        if fmt == "s16" and defect == "no_g":
            Ar, Ai = Ar - 128 * (Gr.sum(0) - Gi.sum(0)), Ai - 128 * (Gr.sum(0) + Gi.sum(0))
        if fmt == "s16" and defect == "g_sign":
            Ar = Ar + 128 * 2 * Gi.sum(0)
        if fmt == "s16" and defect == "wrap32":
            Ar, Ai = ((Ar + 2 ** 31) % 2 ** 32) - 2 ** 31, ((Ai + 2 ** 31) % 2 ** 32) - 2 ** 31
        ar = np.clip((Ar + half) >> shift16, -32768, 32767)
        ai = np.clip((Ai + half) >> shift16, -32768, 32767)
        if stage_a:
            out[chs] = (ar + 1j * ai).T
            continue
        d = np.array([int(incs[c]) for c in chs], np.uint64)
        idx = (((n.astype(np.uint64)[:, None] * d[None, :]) & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.int64)
        c_, s_ = Pt[idx, 0], Pt[idx, 1]
        rr, ri = ar * c_ + ai * s_, ai * c_ - ar * s_
        L = np.array([int(shifts[c]) for c in chs], np.int64)[None, :]
        yr = np.clip((rr + (1 << (21 - L))) >> (22 - L), -128, 127)
        yi = np.clip((ri + (1 << (21 - L))) >> (22 - L), -128, 127)
        rows = np.empty((len(chs), 2 * n_out), np.uint8)
        rows[:, 0::2] = (yr + 128).T.astype(np.uint8)
        rows[:, 1::2] = (yi + 128).T.astype(np.uint8)
        out[chs] = rows
    return out


def from_u8(u8, fmt):
    """the capture of `fmt` that carries the same signal as the offset-binary capture u8: u8 ^ 0x80, or 256 (u8 - 128)"""
    u8 = np.asarray(u8, np.uint8)
    if fmt == "s8":
        return (u8 ^ 0x80).view(np.int8)
    return ((u8.astype(np.int32) - 128) * 256).astype(DTYPE["s16"])
