"""The band activity detector (include/iqdemod.h: "Band activity") as a numpy / Python-int model, written from the
header's text and not from the kernel: a sort for the floor, a walk over the hot bins for the runs.  Every sum is exact
(uint64 holds sum p < 2^43 and sum k p < 2^54).  `defect` switches on one way this can go wrong; the CPU tier
(tests/test_detect_host.py) shows that the GPU test's inputs (tests/detect_cases.py) see each of them."""
from collections import namedtuple

import numpy as np

N_SET = (64, 128, 256, 512, 1024, 2048)
M32 = 2 ** 32 - 1

ROW_DTYPE = np.dtype([("floor", "<u4"), ("threshold", "<u4"), ("n_found", "<u4"), ("n_hot_bins", "<u4")])
DET_DTYPE = np.dtype([("first_bin", "<u4"), ("last_bin", "<u4"), ("peak_bin", "<u4"), ("peak_power", "<u4"),
                      ("sum_power", "<u8"), ("centroid_q8", "<u4"), ("n_hot", "<u4")])
assert ROW_DTYPE.itemsize == 16 and DET_DTYPE.itemsize == 32

Cfg = namedtuple("Cfg", "n_bins floor_rank ratio_q8 dc_guard bridge min_width max_detections")

DEFECTS = [
    "rank_low", "rank_high",          # the floor's rank off by one
    "floor_zero",                     # the floor not raised to 1
    "ge",                             # >= for >
    "prod32",                         # f Q formed in 32 bits
    "no_sat",                         # the threshold cut to 32 bits instead of saturated
    "guard_le_low", "guard_le_high",  # <= for < on either side of the guard
    "guard_in_sums",                  # guard bins above the threshold inside a run enter its sums
    "bridge_low", "bridge_high",      # g - 1, g + 1
    "width_nhot",                     # min_width against n_hot
    "peak_all_bins",                  # the peak over every bin of first .. last
    "peak_tie_high",                  # equal peaks: the highest bin
    "sum32",                          # sum p in 32 bits
    "ksum32",                         # sum k p in 32 bits
    "centroid_round",                 # rounded, not floored
    "found_capped",                   # n_found = min(n_found, K)
    "tail_kept",                      # the records past n_found keep what the buffer held
    "hot_bins_kept_only",             # n_hot_bins without the dropped runs' bins
    "wrap",                           # the run at bin N - 1 joins the run at bin 0
]
STALE = 0xA5                          # what "the buffer held" under tail_kept


def check_cfg(c):
    N = c.n_bins
    assert N in N_SET and 0 <= c.floor_rank < N and 256 <= c.ratio_q8 <= 2 ** 24 and 0 <= c.dc_guard <= N // 4
    assert 0 <= c.bridge <= 64 and 1 <= c.min_width <= N and 1 <= c.max_detections <= N // 2


def threshold(p, c, defect=None):
    """(f, T, the bins above T, the guard bins) of one row"""
    N = c.n_bins
    r = c.floor_rank + {"rank_low": -1, "rank_high": 1}.get(defect, 0)
    f = int(np.sort(p)[min(max(r, 0), N - 1)])
    prod = (f if defect == "floor_zero" else max(f, 1)) * c.ratio_q8
    if defect == "prod32":
        prod &= M32
    T = (prod >> 8) & M32 if defect == "no_sat" else min(M32, prod >> 8)
    k = np.arange(N)
    lo, hi = N // 2 - c.dc_guard, N // 2 + c.dc_guard
    guard = (k >= lo if defect == "guard_le_low" else k > lo) & (k <= hi if defect == "guard_le_high" else k < hi)
    above = p >= T if defect == "ge" else p > T
    return f, T, above, guard


def row_runs(p, c, defect=None):
    """One row: (f, T, n_hot_bins, [run dict]) with every kept run, in ascending first_bin"""
    N = c.n_bins
    p = np.asarray(p).astype(np.uint64)
    assert p.shape == (N,)
    f, T, above, guard = threshold(p, c, defect)
    hot = above & ~guard
    idx = np.flatnonzero(hot)
    g = c.bridge + {"bridge_low": -1, "bridge_high": 1}.get(defect, 0)
    groups = []                                           # the hot bins of each run
    if len(idx):
        cut = np.flatnonzero(np.diff(idx) - 1 > g) + 1
        groups = np.split(idx, cut)
        if defect == "wrap" and len(groups) >= 2 and int(groups[0][0]) + N - int(groups[-1][-1]) - 1 <= g:
            groups = groups[1:-1] + [np.concatenate([groups[-1], groups[0]])]
    runs, hot_kept = [], 0
    for hb in groups:
        first, last = int(hb[0]), int(hb[-1])
        width = (last - first) % N + 1
        if (len(hb) if defect == "width_nhot" else width) < c.min_width:
            continue
        hot_kept += len(hb)
        span = np.arange(first, first + width) % N
        mem = span[above[span]] if defect == "guard_in_sums" else hb
        over = span if defect == "peak_all_bins" else mem
        peak = int(p[over].max())
        at = over[p[over] == peak]
        s = int(p[mem].sum())
        ks = int((p[mem] * mem.astype(np.uint64)).sum())
        if defect == "sum32":
            s = max(s & M32, 1)
        if defect == "ksum32":
            ks &= M32
        cen = (256 * ks + s // 2) // s if defect == "centroid_round" else 256 * ks // s
        runs.append(dict(first_bin=first, last_bin=last, peak_bin=int(at.max() if defect == "peak_tie_high" else at.min()),
                         peak_power=peak, sum_power=s, centroid_q8=cen & M32, n_hot=len(mem)))
    return f, T, (hot_kept if defect == "hot_bins_kept_only" else len(idx)), runs


def detect(power, c, defect=None):
    """power [n_rows, N] uint32 -> (rows [n_rows] ROW_DTYPE, det [n_rows, K] DET_DTYPE): both of the API's arrays in full"""
    check_cfg(c)
    power = np.asarray(power)
    assert power.ndim == 2 and power.shape[1] == c.n_bins and power.dtype == np.uint32
    K = c.max_detections
    rows = np.zeros(len(power), ROW_DTYPE)
    det = np.zeros((len(power), K), DET_DTYPE)
    if defect == "tail_kept":
        det.view(np.uint8)[...] = STALE
    for i, p in enumerate(power):
        f, T, n_hot, runs = row_runs(p, c, defect)
        rows[i] = (f, T, min(len(runs), K) if defect == "found_capped" else len(runs), n_hot)
        for j, r in enumerate(runs[:K]):
            det[i, j] = tuple(r[name] for name in DET_DTYPE.names)
    return rows, det


def offset_hz(n_bins, rate_hz, centroid_q8):
    """iqd_detect_offset_hz: Python's // is the floor division the header asks for"""
    return ((int(centroid_q8) - 128 * n_bins) * int(rate_hz) + 128 * n_bins) // (256 * n_bins)
