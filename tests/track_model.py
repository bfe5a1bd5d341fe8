"""The band activity tracker (include/iqdemod.h: "Band tracks") as a plain Python-int model, written from the header's
text and not from the kernel: a slot is a dict, a block is the header's five steps one after the other.  `defects` switches
on ways this can go wrong (one name or several); the CPU tier (tests/test_track_host.py) shows that the GPU test's inputs
(tests/track_cases.py) see each of them."""
from collections import namedtuple

import numpy as np

from tests import detect_model as dm

N_SET = dm.N_SET
M32 = 2 ** 32 - 1
FREE, TENTATIVE, ACTIVE = 0, 1, 2
F_MATCHED, F_NEW, F_OPENED, F_CLOSED = 1, 2, 4, 8

SLOT_DTYPE = np.dtype([("track_id", "<u4"), ("state", "u1"), ("flags", "u1"), ("hits", "u1"), ("width_class", "u1"),
                       ("misses", "<u2"), ("max_width", "<u2"), ("centre_q8", "<u4"), ("phase_inc", "<u4"),
                       ("first_bin", "<u2"), ("last_bin", "<u2"), ("peak_power", "<u4"), ("age_blocks", "<u4")])
BLOCK_DTYPE = np.dtype([("n_active", "<u4"), ("n_tentative", "<u4"), ("n_opened_closed", "<u4"), ("n_unplaced", "<u4")])
assert SLOT_DTYPE.itemsize == 32 and BLOCK_DTYPE.itemsize == 16

Cfg = namedtuple("Cfg", "n_sources n_bins max_detections n_slots gate_q8 open_hits hold_blocks alpha_q8 inc_bias class_edge")

DEFECTS = [
    "tie_high",               # two slots equally far: the highest index
    "gate_lt",                # < for <= at the gate
    "first_in_gate",          # the first slot in the gate, not the nearest
    "match_twice",            # a matched slot can be matched again in the block (the later detection replaces the earlier)
    "updated_centres",        # a match moves the centre at once and later distances are taken from it
    "shift_trunc",            # the centre's shift truncates toward zero
    "alpha256",               # alpha 256 taken as 255
    "hits_unsat",             # hits wraps at 256
    "open_late",              # open at H + 1 hits
    "close_ge",               # close at misses >= B
    "tentative_survives",     # a tentative slot survives a miss
    "realloc_same_block",     # a slot freed or closed in this block is allocated in it
    "alloc_high",             # allocation takes the highest free slot
    "closed_kept",            # a closed record is not zeroed in the next block
    "flags_kept",             # flags are not cleared
    "age_alloc",              # age counts the allocation block
    "shared_id",              # one next_id for all sources
    "no_carry",               # state is not carried from call to call
    "reset_keeps_id",         # reset leaves next_id
    "read_past_d",            # every one of the row's K records is read
    "found_over_k",           # D = min(n_found, 2 K): past K, into the next row's records
    "inc_sign",               # phase_inc from |centre - 128 N|
    "shift_2048",             # the phase_inc shift of N = 1024 at N = 2048
    "bias_nowrap",            # phase_inc + inc_bias saturates
    "class_last",             # the class from the last width
    "unplaced_zero",          # n_unplaced is not counted
]


def check_cfg(c):
    N = c.n_bins
    assert c.n_sources >= 1 and N in N_SET and 1 <= c.max_detections <= N // 2 and 1 <= c.n_slots <= 64
    assert 0 <= c.gate_q8 < 256 * N and 1 <= c.open_hits <= 255 and 0 <= c.hold_blocks <= 65535 and 1 <= c.alpha_q8 <= 256
    assert 0 <= c.inc_bias <= M32 and len(c.class_edge) == 3
    assert 1 <= c.class_edge[0] <= c.class_edge[1] <= c.class_edge[2] <= N + 1


def phase_inc(n_bins, centre_q8, inc_bias, defects=()):
    """step 5's rule (iqd_track_phase_inc)"""
    log2n = n_bins.bit_length() - 1
    sh = 24 - log2n + (1 if "shift_2048" in defects and n_bins == 2048 else 0)
    d = int(centre_q8) - 128 * n_bins
    if "inc_sign" in defects:
        d = abs(d)
    inc = (d << sh) & M32                                  # Python's & on a negative int is the two's complement mod 2^32
    return min(inc + inc_bias, M32) if "bias_nowrap" in defects else (inc + inc_bias) & M32


ZERO = dict(track_id=0, state=0, flags=0, hits=0, width_class=0, misses=0, max_width=0, centre_q8=0, phase_inc=0,
            first_bin=0, last_bin=0, peak_power=0, age_blocks=0)


class Tracker:
    """One iqd_track object: the slots and next_id of every source, carried from run() to run()."""

    def __init__(self, cfg, defects=()):
        check_cfg(cfg)
        self.cfg = cfg
        self.defects = (defects,) if isinstance(defects, str) else tuple(defects or ())
        assert all(d in DEFECTS for d in self.defects), self.defects
        self.next_id = [0] * cfg.n_sources
        self.reset()

    def reset(self):
        c = self.cfg
        self.slots = [[dict(ZERO) for _ in range(c.n_slots)] for _ in range(c.n_sources)]
        if "reset_keeps_id" not in self.defects:
            self.next_id = [0] * c.n_sources

    def state(self, source):
        out = np.zeros(self.cfg.n_slots, SLOT_DTYPE)
        for s, sl in enumerate(self.slots[source]):
            out[s] = _record(sl)
        return out

    def run(self, rows, det):
        """rows [n_sources, n_blocks] (detect_model.ROW_DTYPE), det [n_sources, n_blocks, K] (detect_model.DET_DTYPE) ->
        (slots [n_sources, n_blocks, S] SLOT_DTYPE, blocks [n_sources, n_blocks] BLOCK_DTYPE)"""
        c, df = self.cfg, self.defects
        rows, det = np.asarray(rows), np.asarray(det)
        assert rows.dtype == dm.ROW_DTYPE and det.dtype == dm.DET_DTYPE
        n_blocks = rows.shape[1]
        assert rows.shape == (c.n_sources, n_blocks) and det.shape == (c.n_sources, n_blocks, c.max_detections) and n_blocks >= 1
        if "no_carry" in df:
            self.reset()
        out = np.zeros((c.n_sources, n_blocks, c.n_slots), SLOT_DTYPE)
        blocks = np.zeros((c.n_sources, n_blocks), BLOCK_DTYPE)
        for j in range(c.n_sources):
            flat = det[j].reshape(-1)
            for b in range(n_blocks):
                n_found, K = int(rows[j, b]["n_found"]), c.max_detections
                D = K if "read_past_d" in df else min(n_found, 2 * K) if "found_over_k" in df else min(n_found, K)
                recs = []
                for i in range(D):
                    r = flat[b * K + i] if b * K + i < len(flat) else np.zeros((), dm.DET_DTYPE)
                    recs.append((int(r["centroid_q8"]), int(r["first_bin"]), int(r["last_bin"]), int(r["peak_power"])))
                ids = 0 if "shared_id" in df else j
                unplaced = self._block(self.slots[j], recs, ids)
                sl = self.slots[j]
                for s in range(c.n_slots):
                    out[j, b, s] = _record(sl[s])
                blocks[j, b] = (sum(x["state"] == ACTIVE for x in sl), sum(x["state"] == TENTATIVE for x in sl),
                                sum(bool(x["flags"] & F_OPENED) for x in sl) | sum(bool(x["flags"] & F_CLOSED) for x in sl) << 16,
                                0 if "unplaced_zero" in df else unplaced)
        return out, blocks

    def _block(self, sl, recs, ids):
        c, df = self.cfg, self.defects
        S, G, H, B = c.n_slots, c.gate_q8, c.open_hits, c.hold_blocks
        A = 255 if "alpha256" in df and c.alpha_q8 == 256 else c.alpha_q8

        def moved(centre, cq):
            d = (cq - centre) * A
            return centre + (-((-d) >> 8) if "shift_trunc" in df and d < 0 else d >> 8)     # >> on a Python int is the floor

        # 0 clear
        for x in sl:
            if x["state"] == FREE and "closed_kept" not in df:
                x.update(ZERO)
            if "flags_kept" not in df:
                x["flags"] = 0
        live0 = [x["state"] != FREE for x in sl]
        free0 = [not v for v in live0]
        centre0 = [x["centre_q8"] for x in sl]
        # 1 match
        match = [None] * S
        unmatched = []
        for i, (cq, _, _, _) in enumerate(recs):
            best = None
            for s in range(S):
                if not live0[s] or (match[s] is not None and "match_twice" not in df):
                    continue
                ref = moved(centre0[s], recs[match[s]][0]) if "updated_centres" in df and match[s] is not None else centre0[s]
                dist = abs(ref - cq)
                if not (dist < G if "gate_lt" in df else dist <= G):
                    continue
                if best is None:
                    best = (dist, s)
                elif "first_in_gate" in df:
                    continue
                elif dist < best[0] or (dist == best[0] and "tie_high" in df):
                    best = (dist, s)
            if best is None:
                unmatched.append(i)
            else:
                match[best[1]] = i
        # 2 update
        for s, x in enumerate(sl):
            if match[s] is None:
                continue
            cq, first, last, peak = recs[match[s]]
            x["centre_q8"] = moved(x["centre_q8"], cq)
            x["first_bin"], x["last_bin"], x["peak_power"] = first, last, peak
            x["max_width"] = max(x["max_width"], last - first + 1)
            x["last_width"] = last - first + 1
            x["hits"] = (x["hits"] + 1) & 255 if "hits_unsat" in df else min(x["hits"] + 1, 255)
            x["misses"] = 0
            x["flags"] |= F_MATCHED
            if x["state"] == TENTATIVE and x["hits"] >= H + ("open_late" in df):
                x["state"] = ACTIVE
                x["flags"] |= F_OPENED
        # 3 age
        for s, x in enumerate(sl):
            if not live0[s]:
                continue
            x["age_blocks"] = (x["age_blocks"] + 1) & M32
            if match[s] is None:
                x["misses"] += 1
                if x["state"] == TENTATIVE:
                    if "tentative_survives" not in df:
                        x.update(ZERO)
                        x.pop("last_width", None)
                elif x["misses"] >= B if "close_ge" in df else x["misses"] > B:
                    x["state"] = FREE
                    x["flags"] |= F_CLOSED
        # 4 allocate
        free = [x["state"] == FREE for x in sl] if "realloc_same_block" in df else free0
        order = [s for s in range(S) if free[s]]
        if "alloc_high" in df:
            order.reverse()
        unplaced = 0
        for i in unmatched:
            if not order:
                unplaced += 1
                continue
            s = order.pop(0)
            cq, first, last, peak = recs[i]
            self.next_id[ids] = (self.next_id[ids] + 1) & M32
            one = H == 1 and "open_late" not in df
            sl[s] = dict(ZERO, track_id=self.next_id[ids], state=ACTIVE if one else TENTATIVE,
                         flags=F_NEW | F_MATCHED | (F_OPENED if one else 0), hits=1, centre_q8=cq, first_bin=first, last_bin=last,
                         peak_power=peak, max_width=last - first + 1, last_width=last - first + 1,
                         age_blocks=1 if "age_alloc" in df else 0)
        # 5 derive
        for x in sl:
            if x["track_id"] != 0:
                x["phase_inc"] = phase_inc(c.n_bins, x["centre_q8"], c.inc_bias, df)
                w = x.get("last_width", x["max_width"]) if "class_last" in df else x["max_width"]
                x["width_class"] = sum(w >= e for e in c.class_edge)
        return unplaced


def _record(x):
    """the fields cut to their widths (misses is stored mod 2^16; a defect may have read garbage)"""
    return tuple(x[n] & (2 ** (8 * SLOT_DTYPE.fields[n][0].itemsize) - 1) for n in SLOT_DTYPE.names)
