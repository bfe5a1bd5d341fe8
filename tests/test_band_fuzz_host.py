"""CPU tier: the fixed slices of tools/band_fuzz.py (the cases tests/test_gpu_band_fuzz.py runs on the GPU) without a GPU.
The slices are the same cases on every machine; every defect of the three models (tests/spectrum_model.py,
tests/detect_model.py, tests/track_model.py) changes the expected arrays of some case of its slice, bar the few that cannot
show inside the specification's bounds; and the slices hold, at least three times each, the structures the kernels'
own code branches on - counted from the drawn inputs and the models' outputs, never from a GPU."""
import hashlib
import os
import sys

import numpy as np
import pytest

from tests import detect_model as dm
from tests import spectrum_model as sm
from tests import track_model as tm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import band_fuzz as bf                                  # noqa: E402

M32 = 2 ** 32 - 1
AT_LEAST = 3

# the drawn parameters of the first cases of every slice (sha256, cut to 16 digits): a change of a generator that changes
# the slices shows here, and is then a decision - the proof and the counts below are run again on the new cases
DIGEST = {"spectrum": "75ddb74efdecc9b1", "detect": "78c4629aa039c5c6", "track": "7ac223d64402e889", "chain": "98596de668b90f20"}
FIRST = {"spectrum": 8, "detect": 12, "track": 10, "chain": 3}


@pytest.fixture(scope="module")
def ctx():
    c = bf.Context(gpu=False)
    yield c
    c.close()


def drawn(kind, n=None):
    seed, cases = bf.SLICES[kind]
    draw = {"spectrum": bf.draw_spectrum, "detect": bf.draw_detect, "track": bf.draw_track, "chain": bf.draw_chain}[kind]
    return [draw(bf.case_rng(seed, i)) for i in range(cases if n is None else n)]


@pytest.fixture(scope="module")
def spectrum_cases():
    return drawn("spectrum")


@pytest.fixture(scope="module")
def detect_cases():
    return drawn("detect")


@pytest.fixture(scope="module")
def track_cases():
    return drawn("track")


def _digest(kind, c):
    h = hashlib.sha256()
    describe = {"spectrum": bf.describe_spectrum, "detect": bf.describe_detect, "track": bf.describe_track, "chain": bf.describe_chain}
    h.update(describe[kind](c).encode())
    if kind == "chain":
        return h                                            # (its capture goes through float sines: the parameters only)
    for key in ("window", "wide", "power", "rows", "det"):
        if c.get(key) is not None:
            h.update(np.ascontiguousarray(c[key]).tobytes())
    return h


@pytest.mark.parametrize("kind", sorted(DIGEST))
def test_slices_are_the_same_cases_every_time(kind):
    a, b = drawn(kind, FIRST[kind]), drawn(kind, FIRST[kind])
    da, db = [_digest(kind, c).hexdigest() for c in a], [_digest(kind, c).hexdigest() for c in b]
    assert da == db
    assert len(set(da)) == len(da)                                        # and they are different cases
    got = hashlib.sha256("".join(da).encode()).hexdigest()[:16]
    assert got == DIGEST[kind], (kind, got)


def test_gpu_false_runs_the_model_alone(ctx):
    """every case function draws its case and runs the model with gpu=False (the context has no engine to run anything on)"""
    assert ctx.eng is None
    for kind, fn in bf.KINDS.items():
        for i in range(2):
            assert fn(bf.case_rng(bf.SLICES[kind][0], i), ctx, gpu=False) is None
    assert all(ctx.stats[k] == 2 for k in ("spectrum cases", "detect cases", "track cases", "chain cases"))


# ---------------------------------------------------------------------------------------------------- the mutation proof

# hi_wrap: |v| <= 32639 holds for every window create accepts, so hi never reaches 128
# (tests/test_spectrum_host.py::test_hi_plane_stays_in_int8_at_the_window_limit_and_wraps_past_it).
# updated_centres: alone it cannot show, a matched slot is out of the loop and nothing reads its centre again in the block
# (tests/test_track_host.py).
EXCUSED = {"spectrum": {"hi_wrap"}, "detect": set(), "track": {"updated_centres"}}


def test_spectrum_slice_sees_every_defect(spectrum_cases, ctx):
    left = set(sm.DEFECTS) - EXCUSED["spectrum"]
    for c in spectrum_cases:
        m = bf.spectrum_model(c, ctx.P)
        want = m.power()
        left -= {d for d in left if not np.array_equal(m.power(d), want)}
        if not left:
            break
    assert not left, left


def test_detect_slice_sees_every_defect(detect_cases):
    left = set(dm.DEFECTS) - EXCUSED["detect"]
    for c in detect_cases:
        want = dm.detect(c["power"], c["cfg"])
        for d in sorted(left):
            got = dm.detect(c["power"], c["cfg"], d)
            if got[0].tobytes() != want[0].tobytes() or got[1].tobytes() != want[1].tobytes():
                left.discard(d)
        if not left:
            break
    assert not left, left


def test_track_slice_sees_every_defect(track_cases):
    left = set(tm.DEFECTS) - EXCUSED["track"]
    for c in track_cases:
        want = c["want"]
        for d in sorted(left):
            got = bf.track_model(c, d)
            if got[0].tobytes() != want[0].tobytes() or got[1].tobytes() != want[1].tobytes():
                left.discard(d)
        if not left:
            break
    assert not left, left


# ---------------------------------------------------------------------------------------------------- structural coverage

def _check(counts, names):
    print(counts)
    low = {k: counts.get(k, 0) for k in names if counts.get(k, 0) < AT_LEAST}
    assert not low, low


def test_spectrum_slice_structures(spectrum_cases):
    n = {}

    def hit(key):
        n[key] = n.get(key, 0) + 1

    for c in spectrum_cases:
        F, rest = c["F"], c["F"] % 64
        hit("N %d" % c["N"])
        hit(c["fmt"])
        hit("F a multiple of 64" if rest == 0 else "tail NT %d" % -(-rest // 16))
        for edge in (16, 17, 32, 33, 48, 49):
            if rest == edge:
                hit("rest %d" % edge)
        if F > 64 and rest:
            hit("F > 64 with a tail")
        if c["n_src"] > 1 and c["blocks"] > 1 and c["N"] >= 128:
            hit("sources, blocks and workgroups per block")
        if c["window"] is not None and c["window"].min() < 0:
            hit("negative window")
        if c["wkind"] == "limit":
            hit("window on the limit")
    _check(n, ["N %d" % N for N in sm.N_SET] + ["u8", "s8", "tail NT 1", "tail NT 2", "tail NT 3", "tail NT 4", "F a multiple of 64",
                                                "F > 64 with a tail", "sources, blocks and workgroups per block", "negative window",
                                                "window on the limit"])


def detect_row_structures(p, cfg, hit):
    N, g, m, K = cfg.n_bins, cfg.bridge, cfg.min_width, cfg.max_detections
    p = p.astype(np.uint64)
    f, T, above, guard = dm.threshold(p, cfg)
    srt = np.sort(p)
    r = cfg.floor_rank
    if (r > 0 and srt[r - 1] == srt[r]) or (r < N - 1 and srt[r + 1] == srt[r]):
        hit("rank inside equal values")
    if f == 0:
        hit("floor 0")
    if T == M32:
        hit("saturated threshold")
    if T >= 2 ** 31:
        hit("threshold >= 2^31")
    idx = np.flatnonzero(above & ~guard)
    if not len(idx):
        hit("row with no hot bin")
        return
    groups = np.split(idx, np.flatnonzero(np.diff(idx) - 1 > g) + 1)
    kept = [int(hb[-1]) - int(hb[0]) + 1 >= m for hb in groups]
    order = np.cumsum(kept) - 1                                           # a kept run's record index
    closes = {}                                                           # word -> the runs that the next run's start closes in it
    for i in range(len(groups) - 1):
        closes.setdefault(int(groups[i + 1][0]) // 64, []).append(i)
    for word, runs in closes.items():
        ks = [kept[i] for i in runs]
        if any(ks) and not all(ks):
            hit("kept and dropped runs close in one word")
        if any(kept[i] and order[i] == K - 1 for i in runs) and any(kept[i] and order[i] >= K for i in runs):
            hit("the K-th and a later kept run close in one word")
    if not kept[-1]:
        hit("last run dropped by min_width")
    elif order[-1] >= K:
        hit("last run is record K + 1 or later")
    for hb, keep in zip(groups, kept):
        if np.any((np.diff(hb) > 1) & (hb[:-1] // 64 != hb[1:] // 64)):
            hit("bridged gap over a multiple of 64")
        if not keep:
            continue
        first, last = int(hb[0]), int(hb[-1])
        if last // 64 - first // 64 >= 2:
            hit("run over three words or more")
        if int(p[hb].sum()) >= 2 ** 32:
            hit("sum_power >= 2^32")
        at = hb[p[hb] == p[hb].max()]
        if at[0] // 64 != at[-1] // 64:
            hit("equal peaks in different words")
        inside = np.arange(first, last + 1)
        if np.any(above[inside] & guard[inside]):
            hit("guard bin above the threshold inside a run")
        if last // 64 - first // 64 >= 2 and at[0] // 64 != at[-1] // 64 and int(p[hb].sum()) >= 2 ** 32 and \
                np.any(above[inside] & guard[inside]):
            hit("three words, a peak tie, a sum above 2^32 and a guard bin in one run")


DETECT_NAMES = ["rank inside equal values", "floor 0", "saturated threshold", "threshold >= 2^31", "row with no hot bin",
                "kept and dropped runs close in one word", "the K-th and a later kept run close in one word",
                "last run dropped by min_width", "last run is record K + 1 or later", "bridged gap over a multiple of 64",
                "run over three words or more", "sum_power >= 2^32", "equal peaks in different words",
                "guard bin above the threshold inside a run",
                "three words, a peak tie, a sum above 2^32 and a guard bin in one run"]


def test_detect_slice_structures(detect_cases):
    n = {}

    def hit(key):
        n[key] = n.get(key, 0) + 1

    for c in detect_cases:
        cfg, rows = c["cfg"], len(c["power"])
        hit("N %d" % cfg.n_bins)
        if rows >= 5 and rows % 4:
            hit("rows mod 4 = %d, two workgroups or more" % (rows % 4))
        seen = set()
        for p in c["power"]:
            detect_row_structures(p, cfg, seen.add)
        for key in seen:                                                  # per case: three cases, not three rows of one case
            hit(key)
    _check(n, ["N %d" % N for N in dm.N_SET] + ["rows mod 4 = %d, two workgroups or more" % r for r in (1, 2, 3)] + DETECT_NAMES)


def track_structures(c, hit):
    """the header's matching walked once more on the drawn arrays, with the model's slots as the state each block starts from"""
    cfg, (slots, blocks) = c["cfg"], c["want"]
    K, S, G = cfg.max_detections, cfg.n_slots, cfg.gate_q8
    resets = set()
    for i, op in enumerate(c["calls"]):
        if op[0] == "reset":
            resets.add(c["calls"][i + 1][1])
    for j in range(cfg.n_sources):
        for b in range(c["n_blocks"]):
            start = slots[j, b - 1] if b and b not in resets else np.zeros(S, tm.SLOT_DTYPE)
            live = start["state"] != tm.FREE
            centre = start["centre_q8"].astype(np.int64)
            n_free = int((~live).sum())
            n_found = int(c["rows"][j, b]["n_found"])
            D = min(n_found, K)
            if n_found > K:
                hit("n_found > K")
            matched = np.zeros(S, bool)
            unmatched, unplaced_first_trip, late = 0, False, set()
            for i in range(D):
                dist = np.abs(centre - int(c["det"][j, b, i]["centroid_q8"]))
                can = live & ~matched
                gate = can & (dist <= G)
                if gate.any():
                    best = dist[gate].min()
                    tie = int((gate & (dist == best)).sum()) >= 2
                    matched[np.flatnonzero(gate & (dist == best))[0]] = True
                    if best == G:
                        hit("distance of exactly G")
                    if tie:
                        hit("two slots equally far")
                    if i >= 64:
                        hit("second trip: a match")
                        if tie:
                            hit("second trip: a tie")
                        if tie or best == G:
                            late.add("edge")
                else:
                    if np.any(can & (dist == G + 1)):
                        hit("distance of G + 1")
                    # An unmatched record i >= 64 can never be placed: the i records before it hold i distinct slots, matched or
                    # allocated, and S <= 64.  What the second trip can get wrong is to place one all the same - the rank
                    # it hands to the free lanes - so the condition is such a record in a block that began with free slots.
                    if i >= 64 and n_free:
                        hit("second trip: an allocation")
                    if unmatched >= n_free:
                        hit("unplaced detections")
                        if i < 64:
                            unplaced_first_trip = True
                    unmatched += 1
            assert max(unmatched - n_free, 0) == int(blocks[j, b]["n_unplaced"])       # the walk is the model's
            if D > 64:
                hit("D > 64")
            if late and unplaced_first_trip:
                hit("second trip: a tie or exactly G behind unplaced detections of the first")
            fl = slots[j, b]["flags"]
            if np.any(fl & tm.F_CLOSED) and np.any(fl & tm.F_NEW):
                hit("a slot closed and another allocated in one block")


TRACK_NAMES = ["S 1", "S 64", "D > 64", "second trip: a match", "second trip: a tie", "second trip: an allocation",    # (see above)
               "second trip: a tie or exactly G behind unplaced detections of the first", "distance of exactly G", "distance of G + 1",
               "two slots equally far", "unplaced detections", "a slot closed and another allocated in one block", "n_found > K",
               "a split call", "a reset between calls", "more than one source"]


def test_track_slice_structures(track_cases):
    n = {}

    def hit(key):
        n[key] = n.get(key, 0) + 1

    for c in track_cases:
        cfg = c["cfg"]
        hit("N %d" % cfg.n_bins)
        if cfg.n_slots in (1, 64):
            hit("S %d" % cfg.n_slots)
        if sum(op[0] == "run" for op in c["calls"]) > 1:
            hit("a split call")
        if any(op[0] == "reset" for op in c["calls"]):
            hit("a reset between calls")
        if cfg.n_sources > 1:
            hit("more than one source")
        seen = set()
        track_structures(c, seen.add)
        for key in seen:                                                  # per case
            hit(key)
    _check(n, ["N %d" % N for N in tm.N_SET] + TRACK_NAMES)


def test_chain_slice_opens_and_closes_tracks(ctx):
    """what tests/test_gpu_band_fuzz.py asserts of the chain slice, shown here first; and both formats, a split call, more
    than one source"""
    seed, cases = bf.SLICES["chain"]
    n = {"opened": 0, "closed": 0, "two calls": 0, "sources > 1": 0, "u8": 0, "s8": 0, "unplaced": 0}
    for i in range(cases):
        c = bf.draw_chain(bf.case_rng(seed, i))
        want = bf.chain_model(c, ctx.P)
        n["opened"] += int((want[4]["n_opened_closed"] & 0xffff).sum())
        n["closed"] += int((want[4]["n_opened_closed"] >> 16).sum())
        n["two calls"] += c["cut"] is not None
        n["sources > 1"] += c["n_src"] > 1
        n[c["fmt"]] += 1
        n["unplaced"] += int(want[4]["n_unplaced"].sum()) > 0
    _check(n, ["opened", "closed", "two calls", "sources > 1", "u8", "s8"])
