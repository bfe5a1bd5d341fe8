"""CPU: the channelizer's edge corpus (tests/chan_corpus.py) and the fuzzer's fixed slices (tools/chan_fuzz.py) have
teeth before they go to the GPU.  Every input runs through the model and through the spec with one defect each
(tests/chan_mutants.py); a defect no input exposes is a kernel bug the GPU tests would pass."""
import os
import sys
import time

import numpy as np
import pytest

from tests import chan_corpus as cc
from tests import chan_model as cm
from tests import chan_mutants as mu
from tests import chan_scan_model as sm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
PATHS = ("K<=256, M even", "K<=256, M odd", "K>256, M even", "K>256, M odd")   # the kernel's four code paths
LOW_BIT = ("a_plus_1", "round_127", "shift_trunc")                             # must show on each of them
OWNS = {"final_tie": ("final_round",), "a_tie_1tap": ("round_127",), "low_order": LOW_BIT, "sat16": ("sat16_wrap",),
        "tap_edges": ("hi_plane", "tap_round"), "general": ("sat8_127", "oldest_tap", "tap_index", "phasor_late", "s_sign")}


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def corpus(capi, P):
    t0 = time.time()
    cases = cc.cases(P, capi.channelizer_default_taps)
    return cases, time.time() - t0


@pytest.fixture(scope="module")
def corpus_kills(corpus, P):
    """{mutant: [cases that expose it]}, and the seconds the whole corpus took through the model and every mutant"""
    cases, t_build = corpus
    t0 = time.time()
    kills = {m: [] for m in mu.MUTANTS}
    for c in cases:
        out = mu.all_outputs(c.wide, c.h, c.M, c.inc, c.L, P)
        assert np.array_equal(out[None], cm.channel(c.wide, c.h, c.M, c.inc, c.L, P)), c   # the restatement is the model
        for m in mu.MUTANTS:
            if not np.array_equal(out[m], out[None]):
                kills[m].append(c)
    return kills, t_build + time.time() - t0


def test_restatement_equals_the_model(corpus, P):
    """mutant=None through the one-call interface, byte for byte, stage a included and on a range of outputs."""
    for c in corpus[0]:
        assert np.array_equal(mu.channel(c.wide, c.h, c.M, c.inc, c.L, P), cm.channel(c.wide, c.h, c.M, c.inc, c.L, P)), c
        a, b = mu.channel(c.wide, c.h, c.M, c.inc, c.L, P, stage_a=True), cm.channel(c.wide, c.h, c.M, c.inc, c.L, P, stage_a=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), c
        r = (c.n_out // 3, c.n_out // 3 + 32)
        assert np.array_equal(mu.channel(c.wide, c.h, c.M, c.inc, c.L, P, m_range=r),
                              cm.channel(c.wide, c.h, c.M, c.inc, c.L, P, m_range=r)), c


def test_every_mutant_is_killed_by_the_corpus(corpus, corpus_kills, capsys):
    cases, _ = corpus
    kills, seconds = corpus_kills
    with capsys.disabled():
        print("\nchannelizer corpus: %d cases through the model and %d mutants in %.1f s" % (len(cases), len(mu.MUTANTS), seconds))
        print("  %-12s %6s   %s" % ("mutant", "cases", "  ".join(PATHS)))
        for m in mu.MUTANTS:
            print("  %-12s %6d   %s" % (m, len(kills[m]), "  ".join(
                "%*d" % (len(p), sum(1 for c in kills[m] if c.path == p)) for p in PATHS)))
    survivors = [m for m in mu.MUTANTS if not kills[m]]
    assert not survivors, "no corpus case exposes: %s" % ", ".join(survivors)
    # every family exposes the defects it was built for (other families may too: no family stands in for another)
    lost = [(f, m) for f, ms in OWNS.items() for m in ms if not any(c.family == f for c in kills[m])]
    assert not lost, "family missing, or blind to the mutant it owns: %r" % lost
    blind = [(m, p) for m in LOW_BIT for p in PATHS if not any(c.path == p for c in kills[m])]
    assert not blind, "a wrong low bit of stage a would pass on: %r" % blind
    assert seconds < 60, seconds


def test_final_rounding_ties_at_every_shift(corpus, P):
    """Unsaturated exact ties of (r + 2^(21-L)) >> (22-L), recounted here from the model's stage a: at every L, on both
    rails and with r of both signs; each moves a byte under the "constant minus one" defect."""
    by_L = {c.L: c for c in corpus[0] if c.family == "final_tie"}
    assert sorted(by_L) == list(range(9))
    for L, c in by_L.items():
        ar, ai = cm.channel(c.wide, c.h, c.M, c.inc, L, P, stage_a=True)
        n = np.arange(c.n_out) * c.M + c.M - 1
        cs = np.array([cc._phasor_at(P, v, c.inc) for v in n], np.int64)
        got = set()
        for rail, r in ((0, ar * cs[:, 0] + ai * cs[:, 1]), (1, ai * cs[:, 0] - ar * cs[:, 1])):
            y = (r + (1 << (21 - L))) >> (22 - L)
            tie = ((r + (1 << (21 - L))) % (1 << (22 - L)) == 0) & (y >= -127) & (y <= 127)
            got |= {(rail, int(np.sign(v))) for v in r[tie]}
        assert got >= {(0, -1), (0, 1), (1, -1), (1, 1)}, (c, got)
        ref = cm.channel(c.wide, c.h, c.M, c.inc, L, P)
        assert not np.array_equal(mu.channel(c.wide, c.h, c.M, c.inc, L, P, mutant="final_round"), ref), c


def test_stage_a_ties_rails_and_the_tap_bound(corpus, P, capsys):
    cases = corpus[0]

    def sums(c):
        Ar, Ai, _ = mu.stage_A(c.wide, c.h, c.M, c.inc, P)
        return np.concatenate([Ar, Ai])

    # exact ties of stage a (A = 128 mod 256), A of both signs: in one-tap cases and inside long filters
    for family, min_k in (("a_tie_1tap", 1), ("low_order", 31)):
        for c in (c for c in cases if c.family == family):
            A = sums(c)
            tie = A[A % 256 == 128]
            assert c.K >= min_k and (tie > 0).any() and (tie < 0).any(), (c, len(tie))
            assert (A % 256 == 127).any() or family == "a_tie_1tap", c          # where A + 1 carries into a
    # low-order visibility: the K and M edges, both operand paths, and hardly a byte on a rail
    low = [c for c in cases if c.family == "low_order"]
    assert {c.K for c in low} >= set(cc.K_EDGES) and {63, 64} <= {c.M for c in low}
    assert {c.path for c in low} == set(PATHS)
    for c in low:
        out = cm.channel(c.wide, c.h, c.M, c.inc, c.L, P)
        assert c.L >= 6 and np.abs(c.h.astype(int)).max() <= 300
        assert ((out == 0) | (out == 255)).mean() < 0.10, c
        ones = next((i for i, u in enumerate(c.cuts) if u != 1), len(c.cuts))
        assert ones * 32 * c.M >= c.K - 1 or c.M >= 32, c      # the history crosses that many shortest calls
    # both int16 rails, the value just past one, and the largest |A| the tap bound allows - inside int32
    top, just = 0, set()
    for c in (c for c in cases if c.family == "sat16"):
        assert np.abs(c.h.astype(np.int64)).sum() == cc.BOUND_SUM
        A = sums(c)
        v = (A + 128) >> 8
        assert (v > 32767).any() and (v < -32768).any(), c
        just |= {int(x) for x in v[(v == 32768) | (v == -32768)]}      # one past the upper rail; the lower rail itself
        top = max(top, int(np.abs(A).max()))
        assert int(np.abs(A).max()) + 128 < 2 ** 31
    with capsys.disabled():
        print("\n  largest |A| of the corpus: %d = 2^31 - %d (256 sum |h| = 2^31 - 256)" % (top, 2 ** 31 - top))
    assert just == {32768, -32768}
    assert top > 2 ** 30                                          # past what taps at 0 degrees alone can reach
    for kind in ("0deg", "45deg"):
        assert 256 * int(np.abs(cc.over_bound_taps(kind).astype(np.int64)).sum()) == 2 ** 31   # one unit over


def test_tap_extremes(corpus, P):
    """h = +-32639 on phasor entries +-32767 and 0; tap bytes -128 and +127 in the lo plane, both ends of the hi plane."""
    g_all = []
    seen = set()
    for c in (c for c in corpus[0] if c.family == "tap_edges"):
        gr, gi = cm.channel_taps(c.h, c.inc, P)
        idx = [((k * c.inc) % (1 << 32)) >> 20 for k in range(c.K)]
        for k in np.flatnonzero(np.abs(c.h.astype(int)) == 32639):
            seen |= {(int(np.sign(c.h[k])), int(P[idx[k]][0])), (int(np.sign(c.h[k])), int(P[idx[k]][1]))}
        g_all += [gr, gi, -gi]                                        # the values the A operands hold
    assert seen >= {(s, p) for s in (-1, 1) for p in (32767, -32767, 0)}, seen
    g = np.concatenate(g_all)
    lo = ((g + 128) % 256) - 128
    hi = (g - lo) // 256
    assert (lo == -128).any() and (lo == 127).any() and hi.max() == 127 and hi.min() <= -127, (hi.min(), hi.max())
    assert np.abs(g).max() > 32512


def test_fuzz_slices_have_teeth(P, capsys):
    """The first channel of every case of the two plain slices, through every mutant: each is exposed by at least three
    cases of each slice.  Exempt are the two the corpus owns (random inputs meet them once or twice in a slice)."""
    import chan_fuzz
    table = {}
    for seed, n in chan_fuzz.SLICES["plain"]:
        rng = np.random.default_rng(seed)
        kills = {m: 0 for m in mu.MUTANTS}
        for _ in range(n):
            for m in chan_fuzz.first_channel_kills(chan_fuzz.draw_plain(rng), P):
                kills[m] += 1
        table[seed] = kills
    with capsys.disabled():
        print("\nchannelizer fuzz slices: cases (of %s) whose first channel exposes the mutant" % (
            ", ".join("%d" % n for _, n in chan_fuzz.SLICES["plain"])))
        print("  %-12s %s" % ("mutant", "  ".join("seed %d" % s for s in table)))
        for m in mu.MUTANTS:
            print("  %-12s %s%s" % (m, "  ".join("%9d" % table[s][m] for s in table),
                                    "   (exempt: the corpus owns it)" if m in mu.EXEMPT_FROM_FUZZ else ""))
    weak = [(s, m, k[m]) for s, k in table.items() for m in mu.MUTANTS if k[m] < 3 and m not in mu.EXEMPT_FROM_FUZZ]
    assert not weak, "fuzz slices expose these in fewer than 3 cases: %r" % weak
    assert set(mu.EXEMPT_FROM_FUZZ) == {"final_round", "sat16_wrap"}


def test_fuzz_draw_is_reproducible_and_in_range():
    import chan_fuzz
    a, b = (chan_fuzz.draw_plain(np.random.default_rng(77)) for _ in range(2))
    assert chan_fuzz.describe(a) == chan_fuzz.describe(b) and np.array_equal(a["wide"], b["wide"])
    rng = np.random.default_rng(78)
    seen_units, seen_k = set(), set()
    for _ in range(200):
        cfg = chan_fuzz.draw_plain(rng)
        h = cfg["h"].astype(np.int64)
        assert 2 <= cfg["M"] <= 64 and 1 <= cfg["K"] <= 1024 and np.abs(h).max() <= 32639 and np.abs(h).sum() <= cc.BOUND_SUM
        assert cfg["src"].max() < cfg["n_src"] and cfg["shift"].max() <= 8 and 1 <= len(cfg["calls"]) <= 8
        assert cfg["wide"].shape == (cfg["n_src"], 64 * cfg["M"] * sum(c["units"] for c in cfg["calls"]))
        tm = chan_fuzz.t_max(cfg["M"], cfg["K"])
        seen_units |= {"min" if c["units"] == 1 else "tail32" if c["units"] % 2 else "even" for c in cfg["calls"]}
        seen_units |= {"windows" for c in cfg["calls"] if c["units"] * 32 > tm}
        seen_k.add(cfg["K"])
    assert seen_units == {"min", "tail32", "even", "windows"} and seen_k >= set(cc.K_EDGES)


def test_scan_mutants_have_teeth(capi, P, oracle):
    """chan_scan_model's wrong models differ from it on a grid that leaves the band and lands on o == Fs/2."""
    from rtlsdrdiags_amd import synth
    M, bo, nb, centre = 4, 128, 8, 1_700_000_000
    fs = 256000 * M
    h = capi.channelizer_default_taps(M)
    wide = synth.wideband(nb * bo * M, fs, [{"offset": 100_000, "kind": "fm", "amplitude": 40.0}], seed=5, sigma=2.0)
    # never opens: one step per block over o = Fs/2 - 2 .. (wrapping to the start); rotation 0: station = centre + o
    grid = (centre + fs // 2 - 2, centre + fs // 2 + 1, 1)

    def run(mutant):
        ch = oracle.chain()
        ch.set_mode("fm")
        ch.set_squelch(0)
        ch.set_rotation(0)
        ch.scanner_set_parameters(*grid)
        ch.scanner_start()
        return sm.follow(ch, wide, h, M, P, 2, centre, bo, nb, rotation=0, mutant=mutant)

    ref = run(None)
    offs = {int(f) - centre for f in ref[4]} | {grid[1] - centre}
    assert {fs // 2 - 1, fs // 2, fs // 2 + 1} <= offs, offs       # the edge itself and both neighbours were cut
    silent = (ref[0].reshape(nb, -1) == 0x80).all(axis=1)
    assert silent.any() and not silent.all()
    for m in sm.SCAN_MUTANTS:
        assert not np.array_equal(run(m)[0], ref[0]), m
    assert sm.tuning(M, centre, centre + fs // 2, 0) is None and sm.tuning(M, centre, centre - fs // 2 - 1, 0) is None
    assert sm.tuning(M, centre, centre - fs // 2, 0) == 2 ** 31 and sm.tuning(M, centre, centre + fs // 2 - 1, 0) < 2 ** 31
