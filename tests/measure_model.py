"""Band track measurements (include/iqdemod.h: "Band track measurements") as a plain model written from the header's text
and not from the kernel: every quantity is a direct sum over the entry's window, bin by bin - no row prefix and no
difference of prefixes, which is the kernel's method.  `defects` switches on ways this can go wrong (one name or several);
the CPU tier (tests/test_measure_host.py) shows that the GPU test's inputs (tests/measure_cases.py) see each of them.
Without a defect the model asserts every bound the header states on every entry it computes."""
from collections import namedtuple

import numpy as np

from tests import detect_model as dm
from tests import track_model as tm

N_SET = dm.N_SET
F_EMPTY, F_WEAK = 1, 2
NONE, CARRIER, NARROW, WIDE = 0, 1, 2, 3

MEAS_DTYPE = np.dtype([("track_id", "<u4"), ("obw_lo", "<u2"), ("obw_hi", "<u2"), ("peak_bin", "<u2"), ("flags", "u1"),
                       ("hint", "u1"), ("peak_excess", "<u4"), ("centroid_q8", "<u4"), ("carrier_q8", "<u2"),
                       ("n_over", "<u2"), ("sum_excess", "<u8")])
assert MEAS_DTYPE.itemsize == 32

Cfg = namedtuple("Cfg", "n_sources n_bins n_slots dc_guard margin obw_tail_q16 carrier_half min_sum carrier_min_q8 wide_bins")

DEFECTS = [
    "floor_kept",             # the floor is not subtracted: e = p where p > f
    "floor_ge",               # >= for > against the floor: a bin at the floor counts in n_over
    "guard_counted",          # guard bins have their excess
    "no_clip_lo",             # the window is not clipped at bin 0: it reads on into what lies before the row
    "no_clip_hi",             # the window is not clipped at bin N - 1: it reads on into what lies behind the row
    "margin_dropped",         # m = 0
    "obw_lo_ge",              # >= for > at the low edge
    "obw_hi_ge",              # >= for > at the high edge
    "beta_total",             # beta is what both ends leave outside together: beta / 2 at each
    "peak_high",              # the highest bin of the maximum
    "carrier_unclipped",      # the carrier's bins are not clipped to the window (only to the row)
    "centroid_rel",           # the centroid counts bins from lo
    "closing_measured",       # a slot in its closing block is measured
    "empty_kept",             # an EMPTY record keeps the window's edges
    "weak_hinted",            # a WEAK record gets its hint
    "hint_order",             # CARRIER is tested before WIDE
    "floor_source0",          # source 0's floor for every source
    "power_prev_block",       # block b's slots with block b - 1's power (block 0: its own)
]


def check_cfg(c):
    N = c.n_bins
    assert c.n_sources >= 1 and N in N_SET and 1 <= c.n_slots <= 64 and 0 <= c.dc_guard <= N // 4 and 0 <= c.margin <= 64
    assert 0 <= c.obw_tail_q16 <= 32767 and 0 <= c.carrier_half <= 8 and 0 <= c.min_sum < 2 ** 32
    assert 0 <= c.carrier_min_q8 <= 256 and 1 <= c.wide_bins <= N + 1


def entry(flat, base, f, t, c, df=()):
    """one entry: flat is the source's power as one list of Python ints, base the index of the row's bin 0, f the floor, t the
    slot (a numpy record).  Returns the record as a dict."""
    N, d, m, beta = c.n_bins, c.dc_guard, 0 if "margin_dropped" in df else c.margin, c.obw_tail_q16
    if "beta_total" in df:
        beta //= 2
    zero = dict.fromkeys(MEAS_DTYPE.names, 0)
    state, tid, first, last = int(t["state"]), int(t["track_id"]), int(t["first_bin"]), int(t["last_bin"])
    if state == 0 and not ("closing_measured" in df and tid != 0):
        return zero
    assert first <= last < N
    lo = first - m if "no_clip_lo" in df else max(first - m, 0)
    hi = last + m if "no_clip_hi" in df else min(last + m, N - 1)

    def p(k):
        i = base + k
        return flat[i] if 0 <= i < len(flat) else 0

    def e(k):
        if not (lo <= k <= hi):
            return 0
        return e_row(k)

    def e_row(k):
        if "guard_counted" not in df and N // 2 - d < k < N // 2 + d:
            return 0
        v = p(k)
        return (v if "floor_kept" in df else v - f) if v > f else 0

    ks = range(lo, hi + 1)
    E = sum(e(k) for k in ks)
    KE = sum(k * e(k) for k in ks)
    n_over = sum(1 for k in ks if e(k) > 0 or ("floor_ge" in df and p(k) == f and not (N // 2 - d < k < N // 2 + d)))
    peak = max(e(k) for k in ks)
    at = [k for k in ks if e(k) == peak]
    peak_bin = at[-1] if "peak_high" in df else at[0]
    out = dict(zero, track_id=tid)
    if E == 0:
        out["flags"] = F_EMPTY
        if "empty_kept" in df:
            out.update(obw_lo=lo, obw_hi=hi, peak_bin=peak_bin)
        return out
    weak = E < c.min_sum
    centroid = (256 * (KE - lo * E if "centroid_rel" in df else KE)) // E
    L, obw_lo = 0, None
    for k in ks:                                                     # L(k) = the sum over lo .. k
        L += e(k)
        if (65536 * L >= beta * E) if "obw_lo_ge" in df else (65536 * L > beta * E):
            obw_lo = k
            break
    R, obw_hi = 0, None
    for k in reversed(ks):                                           # R(k) = the sum over k .. hi
        R += e(k)
        if (65536 * R >= beta * E) if "obw_hi_ge" in df else (65536 * R > beta * E):
            obw_hi = k
            break
    cl, ch = peak_bin - c.carrier_half, peak_bin + c.carrier_half
    if "carrier_unclipped" in df:
        C = sum(e_row(k) for k in range(max(cl, 0), min(ch, N - 1) + 1))
    else:
        C = sum(e(k) for k in range(max(cl, lo), min(ch, hi) + 1))
    carrier = (256 * C) // E
    width = obw_hi - obw_lo + 1
    if "hint_order" in df:
        hint = CARRIER if carrier >= c.carrier_min_q8 else WIDE if width >= c.wide_bins else NARROW
    else:
        hint = WIDE if width >= c.wide_bins else CARRIER if carrier >= c.carrier_min_q8 else NARROW
    if weak and "weak_hinted" not in df:
        hint = NONE
    if not df:                                                       # every bound the header states
        assert 0 <= lo <= obw_lo <= obw_hi <= hi < N and lo <= peak_bin <= hi
        assert 0 < E < 2 ** 43 and KE < 2 ** 54 and 256 * KE < 2 ** 62 and 65536 * E < 2 ** 59 and beta * E < 2 ** 59
        assert 0 <= C <= E and 0 <= carrier <= 256 and 256 * lo <= centroid < 256 * (hi + 1) and 1 <= n_over <= hi - lo + 1
        assert 0 < peak < 2 ** 32 and e(peak_bin) == peak
    out.update(obw_lo=obw_lo, obw_hi=obw_hi, peak_bin=peak_bin, flags=F_WEAK if weak else 0, hint=hint, peak_excess=peak,
               centroid_q8=centroid, carrier_q8=carrier, n_over=n_over, sum_excess=E)
    return out


def measure(power, rows, slots, cfg, defects=()):
    """power [n_sources, n_blocks, N] uint32, rows [n_sources, n_blocks] (detect_model.ROW_DTYPE), slots [n_sources, n_blocks, S]
    (track_model.SLOT_DTYPE) -> [n_sources, n_blocks, S] MEAS_DTYPE"""
    check_cfg(cfg)
    df = (defects,) if isinstance(defects, str) else tuple(defects or ())
    assert all(x in DEFECTS for x in df), df
    power, rows, slots = np.asarray(power), np.asarray(rows), np.asarray(slots)
    assert power.dtype == np.uint32 and rows.dtype == dm.ROW_DTYPE and slots.dtype == tm.SLOT_DTYPE
    J, N, S = cfg.n_sources, cfg.n_bins, cfg.n_slots
    B = rows.shape[1]
    assert power.shape == (J, B, N) and rows.shape == (J, B) and slots.shape == (J, B, S) and B >= 1
    out = np.zeros((J, B, S), MEAS_DTYPE)
    for j in range(J):
        flat = [int(v) for v in power[j].reshape(-1)]
        for b in range(B):
            f = int(rows[0 if "floor_source0" in df else j, b]["floor"])
            pb = max(b - 1, 0) if "power_prev_block" in df else b
            for s in range(S):
                r = entry(flat, pb * N, f, slots[j, b, s], cfg, df)
                out[j, b, s] = tuple(r[n] & (2 ** (8 * MEAS_DTYPE.fields[n][0].itemsize) - 1) for n in MEAS_DTYPE.names)
    return out
