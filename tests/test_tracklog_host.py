"""CPU tier: the band track log (include/iqdemod.h: "Band track log") without a GPU - the mutation proof of the GPU test's
inputs (tests/tracklog_cases.py) on the plain model (tests/tracklog_model.py), what the model's outputs must hold, split calls,
the chained case's events stated by hand, the seeded slice of random scripts, the header's records against the binding's,
iqd_tracklog_mean_centre, and the cross-compiled kernel's code object."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import tracklog_cases as lc
from tests import tracklog_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def models(capi):
    """name -> (case, the model's result): every expected result is computed once"""
    return {c.name: (c, lc.model(c)) for c in lc.cases(capi.channelizer_phasor_table())}


def test_case_list_covers_what_the_kernel_can_get_wrong(models):
    cs = [c for c, _ in models.values()]
    assert [c.name for c in cs] == lc.NAMES
    assert {c.cfg.n_slots for c in cs} >= {1, 8, 64} and {c.cfg.n_sources for c in cs} >= {1, 3}
    assert {op[2] - op[1] for c in cs for op in c.calls if op[0] == "run"} >= {1, 3, 12}
    assert {c.cfg.max_events for c in cs} >= {1, 3, 4, 63, 64}
    stored = [(int(k["n_events"]), c.cfg.max_events) for c, (runs, _) in models.values() for _, _, cnt in runs for k in cnt]
    assert any(n == e for n, e in stored) and any(n == e + 1 for n, e in stored) and (64, 64) in stored and (4, 1) in stored
    flags = set()
    for c, (runs, _) in models.values():
        for summary, events, counts in runs:
            flags |= set(summary["flags"].ravel().tolist()) | set(events["flags"].ravel().tolist())
    assert flags >= {0, lm.F_NEW, lm.F_MODE_CHANGED, lm.F_NEW | lm.F_MODE_CHANGED, lm.F_CLOSED, lm.F_LOST, lm.F_NEW | lm.F_CLOSED}
    hints = np.concatenate([c.meas["hint"][c.slots["track_id"] != 0] for c in cs])
    assert set(hints.tolist()) >= {0, 1, 2, 3, 200}
    mflags = np.concatenate([c.meas["flags"][c.slots["state"] != 0] for c in cs])
    assert set(mflags.tolist()) >= {0, 1, 2}
    assert max(c.slots.nbytes + c.meas.nbytes for c in cs) <= 64 * 24 * 64


# Which cases must see which defect.  A defect not named for a case may still show there; a case is held only to what it was
# planted for.  What the others cannot see by construction:
#   weak_votes, stale_votes   only with a weak (a stale) record in a live block: S8-votes (the chained case's weak records are
#                             the models' own and not planted)
#   tie_high                  only where the top vote is shared when V >= vote_min
#   vote_min_measured         only where a record voted without a hint of 1 .. 3 (hints 0, 200) around vote_min
#   mode_sticky               only where the decision changes after the first one
#   tentative_active, centre_all_live   only with a tentative block
#   first_block_rel           only with a track that starts behind the first call;  state_dropped only with a track over a call
#                             boundary;  reset_kept only with a reset;  g_per_call wherever a track starts behind block 0
#   closing_counted, closed_kept   only with a closing block (closed_kept: and something behind it in the slot)
#   lost_silent, lost_unflagged    only with a vanished track
#   events_descending         only with two events in one block;  events_clipped only with more than E events in a call
#   min_active_off            only with a track that ends at exactly min_active active blocks
MUST_SEE = {
    "weak_votes": ["S8-votes"], "stale_votes": ["S8-votes"], "tie_high": ["S1-life", "S8-votes"],
    "vote_min_measured": ["S1-life", "S8-votes"], "mode_sticky": ["S1-life", "S8-votes", "S8-calls"],
    "tentative_active": ["S1-life", "S8-short-and-lost", "S4-tracker-reset"], "centre_all_live": ["S1-life", "S8-calls"],
    "first_block_rel": ["S8-calls", "J3-sources"], "state_dropped": ["S8-calls", "S8-short-and-lost", "J3-sources", "N256-chained"],
    "reset_kept": ["S8-calls-reset"], "closing_counted": ["S1-life", "S64-burst", "N256-chained"],
    "lost_silent": ["S8-short-and-lost", "S64-burst", "S4-tracker-reset"], "events_descending": ["S8-E4-exact", "S64-burst"],
    "events_clipped": ["S8-E3-over", "S8-E1", "S64-burst-E63"], "min_active_off": ["S8-short-and-lost", "S8-E4-exact"],
    "lost_unflagged": ["S8-short-and-lost", "S64-burst"], "closed_kept": ["S1-life", "S8-calls"],
    "g_per_call": list(lc.NAMES),
}


def test_every_defect_is_seen_by_the_cases_planted_for_it(models):
    """The model with one defect switched on must change some byte of the result on each case named for it."""
    assert sorted(MUST_SEE) == sorted(lm.DEFECTS) and len(lm.DEFECTS) >= 15
    for defect, names in MUST_SEE.items():
        for name in names:
            c, want = models[name]
            assert not lc.same(lc.model(c, defect), want), (defect, name)
    for name, (c, want) in models.items():                                # every case is planted for something
        assert any(name in names for d, names in MUST_SEE.items() if d != "g_per_call"), name
        assert lc.same(lc.model(c), want)


def test_model_outputs_hold_what_the_specification_implies(models):
    """(the model itself asserts the header's bounds on every entry it computes)"""
    for c, (runs, state) in models.values():
        E = c.cfg.max_events
        for summary, events, counts in runs:
            free = summary[summary["track_id"] == 0]
            assert not free.view(np.uint8).any()                          # a free slot: 64 zero bytes
            live = summary[summary["track_id"] != 0]
            assert (live["n_active"] <= live["n_blocks"]).all() and (live["n_measured"] <= live["n_blocks"]).all()
            assert (live["votes"].sum(axis=-1) <= live["n_measured"]).all()
            assert (live["obw_lo_min"][live["n_measured"] == 0] == 0xffff).all()
            assert ((live["flags"] & lm.F_LOST) == 0).all() and ((live["state"] == 0) == ((live["flags"] & lm.F_CLOSED) != 0)).all()
            for j in range(c.cfg.n_sources):
                k = counts[j]
                assert k["n_stored"] == min(int(k["n_events"]), E) and k["n_lost"] <= k["n_events"]
                assert not events[j, k["n_stored"]:].view(np.uint8).any()
                ev = events[j, :k["n_stored"]]
                assert ev["track_id"].all() and (ev["n_active"] >= c.cfg.min_active).all()
                assert (((ev["flags"] & lm.F_LOST) != 0) ^ ((ev["flags"] & lm.F_CLOSED) != 0)).all()
        for j, (st, g) in enumerate(state):
            assert g == sum(op[2] - op[1] for op in c.calls[_last_reset(c.calls):] if op[0] == "run")


def _last_reset(calls):
    at = [i for i, op in enumerate(calls) if op[0] == "reset"]
    return at[-1] + 1 if at else 0


def test_planted_entries_are_what_was_planted(models):
    """S1-life by hand: the vote's course, the sums, the extremes, the event"""
    c, (runs, state) = models["S1-life"]
    summary, events, counts = runs[0]
    s = summary[0, :, 0]
    assert s["mode_hint"].tolist() == [0, 0, 0, 0, 0, 1, 2, 2, 2, 0, 0, 0]
    assert s["flags"].tolist() == [1, 0, 0, 0, 0, 2, 2, 0, 4, 1, 0, 0]
    assert s["n_blocks"].tolist() == [1, 2, 3, 4, 5, 6, 7, 8, 8, 1, 2, 3] and s["n_active"].tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 6, 1, 2, 3]
    assert s["first_block"].tolist() == [0] * 9 + [9] * 3 and s["track_id"].tolist() == [1] * 9 + [2] * 3
    e = events[0, 0]
    assert counts[0].tolist() == (1, 1, 0, 0) and e.tobytes() == s[8].tobytes() and not events[0, 1].tobytes().strip(b"\0")
    assert e["votes"].tolist() == [2, 3, 1] and e["n_measured"] == 8
    assert e["sum_centre_q8"] == 5020 + 5100 + 4900 + 5000 + 5050 + 5060 and e["sum_excess"] == 2 * (2 ** 43 - 1) + 5 + 7 + 9 + 11 + 13 + 15
    assert (e["peak_excess"], e["obw_lo_min"], e["obw_hi_max"]) == (2 ** 32 - 1, 29, 65535)
    assert state[0][0][0]["track_id"] == 2 and state[0][1] == 12
    # 64 events in one block, in slot order, closed and lost alternating
    _, (runs, _) = models["S64-burst"]
    _, events, counts = runs[0]
    assert counts[0].tolist() == (64, 64, 0, 32) and events[0]["track_id"].tolist() == list(range(100, 164))
    assert events[0]["flags"].tolist() == [lm.F_CLOSED, lm.F_LOST] * 32
    _, (runs, _) = models["S64-burst-E63"]
    assert runs[0][2][0].tolist() == (64, 63, 0, 32) and runs[0][1][0]["track_id"].tolist() == list(range(100, 163))
    # LOST and NEW in one block, across a call boundary
    _, (runs, _) = models["S8-short-and-lost"]
    summary, events, counts = runs[1]
    assert (summary[0, 0, 3]["track_id"], summary[0, 0, 3]["flags"], summary[0, 0, 3]["first_block"]) == (5, lm.F_NEW, 3)
    assert (events[0, 0]["track_id"], events[0, 0]["flags"], events[0, 0]["n_active"]) == (3, lm.F_CLOSED, 3)   # slot 2, same block
    assert (events[0, 1]["track_id"], events[0, 1]["flags"], events[0, 1]["n_active"]) == (4, lm.F_LOST, 3)
    # events: 3 closed, 4 lost, 10 lost, 12 closed, 11 lost; short: 2 (two active blocks), 5 (two), 13 (seen closing only)
    assert events[0, :5]["track_id"].tolist() == [3, 4, 10, 12, 11]
    assert counts[0].tolist() == (5, 5, 3, 3) and runs[0][2][0].tolist() == (0, 0, 1, 0)


def test_the_chained_cases_events_fall_where_the_stations_were_keyed(capi, models):
    """The keyed capture through the five models.  By hand: the AM station at +250 kHz is keyed on over blocks 6.5 .. 14.3, so
    the detector sees it from block 6 on and through block 14; the tracker (open_hits 3, hold_blocks 2) makes it tentative
    in 6 and 7, active from 8, holds it over 15 and 16 and closes it in 17 - the one event, in the second call (blocks
    10 .. 19): slot 1, id 2, first seen in block 6, 11 live blocks of which 9 active, CARRIER.  The FM station at -700 kHz is
    on throughout: never an event, open at the end with 24 blocks of which 22 active."""
    from tests import detect_model as dm
    from tests import track_cases as tc
    c, (runs, state) = models["N256-chained"]
    N = tc.CHAINED["N"]
    assert [r[2][0].tolist() for r in runs] == [(0, 0, 0, 0), (1, 1, 0, 0), (0, 0, 0, 0)]
    e = runs[1][1][0, 0]
    assert (e["track_id"], e["first_block"], e["n_blocks"], e["n_active"], e["flags"], e["state"]) == (2, 6, 11, 9, lm.F_CLOSED, 0)
    assert e.tobytes() == runs[1][0][0, 17 - 10, 1].tobytes()             # the closing block's record of slot 1
    assert e["mode_hint"] == 1 and e["votes"][0] >= 6 and e["n_measured"] >= 7
    am = dm.offset_hz(N, tc.RATE, capi.tracklog_mean_centre(int(e["sum_centre_q8"]), int(e["n_active"])))
    assert abs(am - 250000) <= tc.RATE / N
    live, g = state[0]
    assert g == 24 and live["track_id"].tolist() == [1, 0, 0, 0]
    o = live[0]
    assert (o["first_block"], o["n_blocks"], o["n_active"], o["state"], o["flags"]) == (0, 24, 22, 2, 0)
    fm = dm.offset_hz(N, tc.RATE, capi.tracklog_mean_centre(int(o["sum_centre_q8"]), int(o["n_active"])))
    assert abs(fm + 700000) <= tc.RATE / N


def _one_call(c, E):
    cfg = c.cfg._replace(max_events=E)
    log = lm.TrackLog(cfg)
    return log.run(c.slots, c.meas), [log.state(j) for j in range(cfg.n_sources)]


def test_split_calls_give_the_one_calls_result(models):
    """a call of b1 + b2 blocks: the summaries of a call of b1 followed by one of b2, the events concatenated, the counts
    summed (E large enough) - for every case without a reset, at every cut and block by block"""
    for c, _ in models.values():
        if any(op[0] == "reset" for op in c.calls):
            continue
        E, B, J = 256, c.n_blocks, c.cfg.n_sources
        (summary, events, counts), state = _one_call(c, E)
        cuts = [[0, k, B] for k in range(1, B)] + [list(range(B + 1))]
        for cut in cuts:
            log = lm.TrackLog(c.cfg._replace(max_events=E))
            parts = [log.run(c.slots[:, a:b], c.meas[:, a:b]) for a, b in zip(cut, cut[1:])]
            assert np.concatenate([p[0] for p in parts], axis=1).tobytes() == summary.tobytes(), (c.name, cut)
            for j in range(J):
                ev = np.concatenate([p[1][j, :p[2][j]["n_stored"]] for p in parts])
                assert ev.tobytes() == events[j, :counts[j]["n_stored"]].tobytes(), (c.name, cut, j)
                for f in lm.COUNTS_DTYPE.names:
                    assert sum(int(p[2][j][f]) for p in parts) == counts[j][f]
                assert log.state(j)[0].tobytes() == state[j][0].tobytes() and log.state(j)[1] == state[j][1]


def test_the_seeded_slice_holds_enough_of_every_kind():
    """the 200 random scripts of the GPU test: the shapes the issue names, and at least ten cases each of an overflowing
    call, a LOST event, a decision on a tie of votes and a track that spans a call boundary"""
    cs = lc.fuzz_cases()
    assert len(cs) == 200 and len({c.name for c in cs}) == 200
    assert {c.cfg.n_slots for c in cs} == {1, 5, 64} and {c.cfg.n_sources for c in cs} == {1, 2, 3}
    runs = [[op[2] - op[1] for op in c.calls if op[0] == "run"] for c in cs]
    assert {len(r) for r in runs} == {1, 2, 3, 4} and {n for r in runs for n in r} == set(range(1, 10))
    assert any(op[0] == "reset" for c in cs for op in c.calls)
    n = dict.fromkeys(("overflow", "lost", "tie", "span"), 0)
    for c in cs:
        for k in lc.kinds(c, lc.model(c)):
            n[k] += 1
    assert min(n.values()) >= 10, n
    again = lc.random_case(lc.FUZZ_SEED, 17)
    assert again.slots.tobytes() == cs[17].slots.tobytes() and again.meas.tobytes() == cs[17].meas.tobytes()


def test_structures_are_the_headers(capi):
    assert capi.TRACK_SUMMARY == lm.SUMMARY_DTYPE and capi.TRACK_SUMMARY.itemsize == 64 and C.sizeof(capi.TrackLogConfig) == 32
    assert capi.TRACKLOG_COUNTS == lm.COUNTS_DTYPE and capi.TRACKLOG_COUNTS.itemsize == 16
    assert [capi.TRACK_SUMMARY.fields[n][1] for n in capi.TRACK_SUMMARY.names] == [0, 4, 5, 6, 7, 8, 16, 20, 24, 28, 40, 48, 56, 60, 62]
    header = open(os.path.join(ROOT, "include", "iqdemod.h")).read()
    assert "Band track log" in header
    for struct, names in (("iqd_track_summary", capi.TRACK_SUMMARY.names), ("iqd_tracklog_counts", capi.TRACKLOG_COUNTS.names),
                          ("iqd_tracklog_config", [f[0] for f in capi.TrackLogConfig._fields_])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        got = [re.sub(r"\[\d+\]", "", n).strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert got == list(names), struct
    for name, value in (("IQD_TLOG_F_NEW", lm.F_NEW), ("IQD_TLOG_F_MODE_CHANGED", lm.F_MODE_CHANGED), ("IQD_TLOG_F_CLOSED", lm.F_CLOSED),
                        ("IQD_TLOG_F_LOST", lm.F_LOST)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert (capi.TLOG_F_NEW, capi.TLOG_F_MODE_CHANGED, capi.TLOG_F_CLOSED, capi.TLOG_F_LOST) == (1, 2, 4, 8)
    assert re.search(r"#define IQD_ABI_VERSION 1\b", header)
    for name in ("iqd_tracklog_create", "iqd_tracklog_destroy", "iqd_tracklog_reset", "iqd_tracklog_run_device", "iqd_tracklog_run",
                 "iqd_tracklog_get_state", "iqd_tracklog_mean_centre"):
        assert name in capi.EXPORTS and getattr(capi._lib(), name)
    assert capi.tracklog_defaults() == dict(min_active=2, vote_min=4, max_events=256)


def test_mean_centre_is_the_formula(capi):
    rng = np.random.default_rng(5)
    pairs = [(0, 1), (1, 1), (2 ** 51 - 1, 2 ** 32 - 1), (2 ** 51 - 1, 1 << 20), (2 ** 19 - 1, 1), (7, 8), ((2 ** 32 - 1) ** 2 + 5, 2 ** 32 - 1),
             ((2 ** 32 - 1) * 77 + 76, 77)]
    pairs += [(int(rng.integers(0, 2 ** 51)), int(rng.integers(1 << 19, 2 ** 32))) for _ in range(50)]
    pairs += [(n * int(rng.integers(0, 2 ** 19)) + int(rng.integers(0, n)), n) for n in (1, 2, 3, 1000, 65535)]
    for total, n in pairs:
        assert capi.tracklog_mean_centre(total, n) == total // n, (total, n)
    for total, n in ((5, 0), (2 ** 64 - 1, 2 ** 32 - 1), (2 ** 32 * 77, 77)):        # n = 0; a quotient that 32 bits do not hold
        with pytest.raises(capi.IqdError):
            capi.tracklog_mean_centre(total, n)
    L = capi._lib()
    assert L.iqd_tracklog_mean_centre(5, 1, None) == -1 and L.iqd_tracklog_mean_centre(5, 0, C.byref(C.c_uint32())) == -1


KERNEL = "_ZN3iqd10tlg_kernelENS_9TlgLaunchE"


@pytest.fixture(scope="module")
def code_object():
    """iqd_tracklog.hip cross-compiled for gfx950 (device only, the library's flags): {kernel: metadata}"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "iqd_tracklog.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
               os.path.join(csrc, "iqd_tracklog.hip")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(asm).read()
        for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
            kernel = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[kernel] = {k: int(v) for k, v in re.findall(
                r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\d+)", blk)}
    return meta


def test_code_object(code_object):
    """one kernel, registers only: no private segment, no spills, no LDS; the counts DESIGN 4.16 records (77 VGPRs, 52 SGPRs
    when this was written) with room for a compiler's mood"""
    assert sorted(code_object) == [KERNEL]
    m = code_object[KERNEL]
    print("tlg_kernel:", m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == 0, m
    assert m["vgpr_count"] <= 96 and m["sgpr_count"] <= 80, m


def test_isa_lint_of_the_tracklog_kernel():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_tracklog.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 1 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
