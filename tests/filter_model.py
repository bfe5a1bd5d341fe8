"""numpy model of the four stand-alone filter kinds (include/iqdemod.h: iqd_filter_*), call by call with the state the
kernels carry, and with switchable defects for the mutation proof of tests/test_filter_host.py.

  decimate_i16 / fir_i16  Decimator_int16.cc:176-238, FirFilter_int16.cc:151-213
  fir_f32                 FirFilter.cc:144-185
  iir_f32                 IirFilter.cc:161-229

run(kind, num, den, factor, x, cuts, defect) -> [n_ch, n_out]; x is [n_ch, N], cuts the call boundaries [0, .., N]."""
import numpy as np

Q15_KINDS = ("decimate_i16", "fir_i16")
DEFECTS = {
    "clamp_end": "clamp only after the last tap",
    "clamp_hi": "upper clamp 2^30 instead of 2^30 - 1",
    "no_round": "no rounding term",
    "div": "division by 32768 instead of an arithmetic shift",
    "emit0": "an output on n = 0 (mod factor) instead of n = factor - 1",
    "hist_zero": "history zeroed at every call",
    "taps_rev": "taps reversed",
    "desc_k": "float sum in descending k",
    "fma": "fused multiply-add: the product in float64, one rounding",
    "rec_add": "IIR recursive part added instead of subtracted",
    "y_shift": "IIR using y[n-k] instead of y[n-1-k]",
    "state_drop": "IIR state not carried across calls",
    "chan0": "channel c reading channel 0's state",
}
_APPLIES = {
    "decimate_i16": {"clamp_end", "clamp_hi", "no_round", "div", "emit0", "hist_zero", "taps_rev", "chan0"},
    "fir_i16": {"clamp_end", "clamp_hi", "no_round", "div", "hist_zero", "taps_rev", "chan0"},
    "fir_f32": {"hist_zero", "taps_rev", "desc_k", "fma", "chan0"},
    "iir_f32": {"taps_rev", "desc_k", "fma", "rec_add", "y_shift", "state_drop", "chan0"},
}


def applies(defect, kind):
    return defect in _APPLIES[kind]


def quantize(h):
    """the reference constructors' Q15 quantisation: round(32768 h) cast to int16 (1.0 -> -32768)"""
    s = np.asarray(h, np.float32) * np.float32(32768)
    r = np.where(s >= 0, np.floor(s + np.float32(0.5)), np.ceil(s - np.float32(0.5)))      # roundf: halves away from zero
    return (r.astype(np.int64) & 0xffff).astype(np.uint16).view(np.int16)


def clamp_free_taps(hq):
    """the largest K0 with sum_{k < K0} |hq[k]| <= 32767"""
    c = np.cumsum(np.abs(np.asarray(hq, np.int64)))
    return int(np.searchsorted(c, 32767, side="right"))


def _mac_f32(y, h, x, defect):
    if defect == "fma":
        return (y.astype(np.float64) + np.float64(h) * x.astype(np.float64)).astype(np.float32)
    return y + np.float32(h) * x


def _fir_positions(kind, factor, count, n_in, defect):
    """call-relative input indices of the call's outputs; count = samples before the call"""
    if kind != "decimate_i16":
        return np.arange(n_in)
    want = 0 if defect == "emit0" else factor - 1
    first = (want - count) % factor
    return np.arange(first, n_in, factor)


def _run_fir(kind, num, factor, x, cuts, defect):
    n_ch = x.shape[0]
    q15 = kind in Q15_KINDS
    h = quantize(num).astype(np.int64) if q15 else np.asarray(num, np.float32)
    if defect == "taps_rev":
        h = h[::-1]
    L = len(h)
    dt = np.int64 if q15 else np.float32
    hist = np.zeros((n_ch, L - 1), dt)
    outs = []
    order = range(L - 1, -1, -1) if defect == "desc_k" else range(L)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if defect == "hist_zero":
            hist = np.zeros_like(hist)
        src = np.broadcast_to(hist[:1], hist.shape) if defect == "chan0" else hist
        xx = np.concatenate([src, x[:, a:b].astype(dt)], axis=1)
        pos = _fir_positions(kind, factor, a, b - a, defect) + (L - 1)
        if q15:
            acc = np.full((n_ch, len(pos)), 0 if defect == "no_round" else 1 << 14, np.int64)
            hi = (1 << 30) if defect == "clamp_hi" else (1 << 30) - 1
            for k in range(L):
                acc = acc + h[k] * xx[:, pos - k]
                if defect != "clamp_end" or k == L - 1:
                    acc = np.clip(acc, -(1 << 30), hi)
            y = np.trunc(acc / 32768.0).astype(np.int64) if defect == "div" else acc >> 15
            outs.append((y & 0xffff).astype(np.uint16).view(np.int16))
        else:
            y = np.zeros((n_ch, len(pos)), np.float32)
            for k in order:
                y = _mac_f32(y, h[k], xx[:, pos - k], defect)
            outs.append(y)
        full = np.concatenate([hist, x[:, a:b].astype(dt)], axis=1)
        hist = full[:, full.shape[1] - (L - 1):]
    return np.concatenate(outs, axis=1) if outs else np.zeros((n_ch, 0), np.int16 if q15 else np.float32)


def _run_iir(num, den, x, cuts, defect):
    n_ch = x.shape[0]
    b, a = np.asarray(num, np.float32), np.asarray(den, np.float32)
    if defect == "taps_rev":
        b, a = b[::-1], a[::-1]
    nb, na = len(b), len(a)
    x = np.asarray(x, np.float32)
    out = np.zeros_like(x)
    zero = np.zeros(n_ch, np.float32)
    xs, ys = [zero] * (nb - 1), [zero] * na              # xs[i] = x[n-1-i], ys[i] = y[n-1-i]
    kb = range(nb - 1, -1, -1) if defect == "desc_k" else range(nb)
    ka = range(na - 1, -1, -1) if defect == "desc_k" else range(na)
    with np.errstate(all="ignore"):
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if defect == "state_drop":
                xs, ys = [zero] * (nb - 1), [zero] * na
            if defect == "chan0":
                xs = [np.full(n_ch, v[0], np.float32) for v in xs]
                ys = [np.full(n_ch, v[0], np.float32) for v in ys]
            for n in range(lo, hi):
                xin = [x[:, n]] + xs
                v = zero
                for k in kb:
                    v = _mac_f32(v, b[k], xin[k], defect)
                yin = ([zero] + ys) if defect == "y_shift" else ys      # y[n] itself is not there yet: it reads 0
                r = zero
                for k in ka:
                    r = _mac_f32(r, a[k], yin[k], defect)
                y = v + r if defect == "rec_add" else v - r
                out[:, n] = y
                xs = xin[:nb - 1]
                ys = ([y] + ys)[:na]
    return out


def run(kind, num, den, factor, x, cuts=None, defect=None):
    assert defect is None or defect in DEFECTS
    x = np.atleast_2d(x)
    cuts = [0, x.shape[1]] if cuts is None else list(cuts)
    assert cuts[0] == 0 and cuts[-1] == x.shape[1] and all(a <= b for a, b in zip(cuts[:-1], cuts[1:]))
    if kind == "iir_f32":
        return _run_iir(num, den, x, cuts, defect)
    return np.ascontiguousarray(_run_fir(kind, num, factor, x, cuts, defect))
