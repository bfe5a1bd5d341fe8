"""CPU tier for track-following wideband channels (include/iqdemod.h: "Track-following channels"): the mutation proof of the
GPU test's inputs (tests/chan_track_cases.py) on the numpy model (tests/chan_track_model.py), the model's own call-split
identity, the chained case against where its stations were put, and the cross-compiled kernels' code object."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import chan_model as cm
from tests import chan_track_cases as tc
from tests import chan_track_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def cases(capi, P):
    return tc.cases(capi, P)


# The defects a case cannot see, by construction.
NO_SCRIPT = {"carry_over_reset", "carry_at_start"}     # the cases of plain runs neither reset nor stop and start
LAG0 = {"carry_dropped", "carry_lagged"}               # at lag 0 no block reads the carry
ONE_WINDOW = {"bound_window"}                          # a block that fits one window has no window boundary inside
WHOLE_64 = {"bound_64"}                                # block_bytes a multiple of 128: every boundary is a multiple of 64 outputs
ONE_SOURCE = {"source0"}
BLIND = {
    "M8-1f-S1-b64": NO_SCRIPT | LAG0 | ONE_WINDOW | ONE_SOURCE | {"ch_as_slot"},   # S = 1: every index is slot 0
    "M8-7f-S8-b256-script": ONE_WINDOW | WHOLE_64 | ONE_SOURCE,
    "M2-9f-S8-b256": NO_SCRIPT | ONE_WINDOW | WHOLE_64 | {"min_state_ignored"},    # min_state 1: nothing to ignore
    "M7-65f-S64-b1024": NO_SCRIPT | LAG0 | ONE_WINDOW | WHOLE_64 | {"min_state_ignored"},
    "K300-9f-S8-b256": NO_SCRIPT | ONE_WINDOW | WHOLE_64 | ONE_SOURCE,
    "M8-9f-S8-b2560": NO_SCRIPT | WHOLE_64 | ONE_SOURCE,
    # One block per call at lag 1: the call's only block is cut with the carry.  The entry one late is the carry as well; the
    # previous block's decision is the carry, i.e. the block's own, so swapping taps and rotation between the two changes
    # nothing; and the call's first block is every block.
    "M8-7f-S8-b256-1blk": NO_SCRIPT | ONE_WINDOW | WHOLE_64 | ONE_SOURCE | {"late", "taps_held", "new_taps_old_rot", "old_taps_new_rot"},
    # the tracker's own table: one source, slot s on channel s (of S = 4 channels), lag 0
    "M8-chained": NO_SCRIPT | LAG0 | ONE_WINDOW | WHOLE_64 | ONE_SOURCE | {"ch_as_slot"},
}


def test_every_gpu_input_sees_every_defect(capi, P, cases):
    seen_anywhere = set()
    for case in cases:
        fol = [int(c) for c in np.nonzero(case.slot >= 0)[0]]
        w = tc.window_of(capi, case)
        truth = {c: np.concatenate(tc.run_model(tm, cm, case, P, c, window=w)) for c in fol}
        seen = set()
        for d in tm.DEFECTS:
            for c in fol:
                if not np.array_equal(np.concatenate(tc.run_model(tm, cm, case, P, c, defect=d, window=w)), truth[c]):
                    seen.add(d)
                    break
        blind = set(tm.DEFECTS) - seen
        assert blind == BLIND[case.name], (case.name, blind ^ BLIND[case.name])
        seen_anywhere |= seen
    assert seen_anywhere == set(tm.DEFECTS)


def test_a_call_split_in_two_equals_the_whole(P, cases):
    """lag 1: 12 blocks in one call, as 5 + 7 and as twelve calls, the table cut alike"""
    case = {c.name: c for c in cases}["M2-9f-S8-b256"]
    assert case.lag == 1 and case.nblk == 12
    for c in np.nonzero(case.slot >= 0)[0][:4]:
        res = []
        for cuts in ([12], [5, 7], [1] * 12):
            f = tm.Follower(case.h, case.M, P, case.src[c], case.shift[c], case.slot[c], channel=c)
            rows, b = [], 0
            for n in cuts:
                rows.append(f.call(case.wide[case.src[c]], case.table[:, b:b + n], case.bb, 1, case.min_state))
                b += n
            res.append(np.concatenate(rows))
        assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[2])
        assert len(set(res[0].tolist())) > 2


def test_the_cases_reach_what_they_are_for(capi, P, cases):
    by = {c.name: c for c in cases}
    assert {c.M for c in cases} >= {2, 7, 8} and {int((c.slot >= 0).sum()) for c in cases} >= {1, 7, 9, 65}
    assert {c.S for c in cases} >= {1, 8, 64} and {c.bb for c in cases} >= {64, 256, 1024, 2560}
    assert {c.nblk for c in cases} >= {1, 3, 12} and {c.lag for c in cases} == {0, 1} and {c.min_state for c in cases} == {1, 2}
    assert (len(by["K300-9f-S8-b256"].h) + 31) // 32 > 8                # more K-chunks than stay in registers
    c = by["M2-9f-S8-b256"]
    assert c.n_src == 3 and 1 not in set(c.src[c.slot >= 0].tolist()) and 1 in set(c.src.tolist())   # a source with fixed channels only
    assert sum(1 for c in cases if (c.slot < 0).any()) >= 4             # fixed channels beside followers
    c = by["M8-9f-S8-b2560"]                                            # a block of more outputs than one window holds
    w = tc.window_of(capi, c)
    assert capi.channelizer_track_window_outputs(c.M, len(c.h)) <= capi.channelizer_window_outputs(c.M, len(c.h))
    assert 0 < w < c.bb // 2 and c.bb // 2 % w
    for c in cases:
        assert c.wide.shape == (c.n_src, c.ncalls * c.nblk * c.bb * c.M) and c.table.shape == (c.n_src, c.ncalls * c.nblk, c.S)
        assert c.nblk * c.bb % tc.ENGINE_BB == 0 and c.bb % 64 == 0
        if c.name == "M8-chained":
            continue
        fol = np.nonzero(c.slot >= 0)[0]
        kinds = set()
        for ch in fol:
            kinds |= set(tc.kind_of(c.table[c.src[ch], :, c.slot[ch]]).tolist())
        assert kinds == {tc.FREE, tc.TENTATIVE, tc.ACTIVE, tc.CLOSING}, c.name
        incs = np.concatenate([c.table["phase_inc"][c.src[ch], :, c.slot[ch]][c.table["state"][c.src[ch], :, c.slot[ch]] == 2] for ch in fol])
        assert set(tc.SPECIAL) <= set(incs.tolist()), c.name            # 0, 0x80000000 and 0xffffffff in live blocks
        for ch in fol:                                                  # and otherwise new in every block
            seq = [int(v) for v in c.table["phase_inc"][c.src[ch], :, c.slot[ch]][c.table["state"][c.src[ch], :, c.slot[ch]] == 2]
                   if int(v) not in tc.SPECIAL]
            assert len(set(seq)) == len(seq), (c.name, ch)
        if len(fol) > 1:                                                # two channels on one slot
            pairs = [(int(c.src[ch]), int(c.slot[ch])) for ch in fol]
            assert len(set(pairs)) < len(pairs), c.name
    rows = np.concatenate([np.concatenate(tc.run_model(tm, cm, by["K300-9f-S8-b256"], P, int(ch)))
                           for ch in np.nonzero(by["K300-9f-S8-b256"].slot >= 0)[0]])
    assert rows.min() == 0 and rows.max() == 255                        # the output's rails


def test_the_chained_case_is_live_where_and_when_its_stations_are(P, cases):
    from tests import track_cases as trc
    case = {c.name: c for c in cases}["M8-chained"]
    c = trc.CHAINED
    N, F, nb = c["N"], c["F"], c["blocks"]
    state, inc = case.table["state"][0], case.table["phase_inc"][0]
    hz = ((inc.astype(np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31) * trc.RATE / 2 ** 32
    live = state >= 2
    found = {}
    for s in range(case.S):
        if live[:, s].any():
            f = float(np.median(hz[live[:, s], s]))
            found[min(trc.STATIONS, key=lambda st: abs(st["offset"] - f))["offset"]] = (s, f)
    assert set(found) == {-700e3, 250e3}, found
    for off, (s, f) in found.items():
        assert abs(f - off) <= trc.RATE / N, (off, f)                   # within a bin of the station
    s_fm, s_am = found[-700e3][0], found[250e3][0]
    assert live[:, s_fm].tolist() == [b >= c["H"] - 1 for b in range(nb)]   # always on: open at its third hit, then for good
    on = np.nonzero(live[:, s_am])[0]
    first_full, last_any = int(np.ceil(6.5)), int(14.3)                     # keyed over samples [6.5, 14.3) N F
    assert on.min() in (first_full + c["H"] - 2, first_full + c["H"] - 1) and last_any <= on.max() <= last_any + c["B"]
    assert np.array_equal(on, np.arange(on.min(), on.max() + 1))
    # the rows: silence exactly in the blocks that are not live, something else in the live ones
    for s in (s_fm, s_am):
        row = np.concatenate(tc.run_model(tm, cm, case, P, s)).reshape(nb, case.bb)
        assert [bool((row[b] == 0x80).all()) for b in range(nb)] == [not v for v in live[:, s]]


@pytest.fixture(scope="module")
def code_object():
    """iqd_chan_track.hip cross-compiled for gfx950 (device only, the library's flags): {kernel: metadata}"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "iqd_chan_track.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
               os.path.join(csrc, "iqd_chan_track.hip")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        for blk in re.split(r"\n\s+- \.agpr_count:", open(asm).read())[1:]:
            kernel = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[kernel] = {k: int(v) for k, v in re.findall(
                r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", blk)}
    return meta


def test_code_object_of_the_track_kernels(code_object):
    reg, big, build = ("_ZN3iqd16chz_track_kernelILi8EEEvNS_9ChzLaunchENS_14ChzTrackLaunchE",
                       "_ZN3iqd16chz_track_kernelILi0EEEvNS_9ChzLaunchENS_14ChzTrackLaunchE",
                       "_ZN3iqd22chz_track_build_kernelENS_9ChzLaunchENS_14ChzTrackLaunchE")
    assert sorted(code_object) == sorted([reg, big, build])
    for k, m in code_object.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
    assert code_object[reg]["vgpr_count"] <= 128, code_object[reg]         # two workgroups of 512 per CU, like chz_kernel
    got = {k: code_object[k]["vgpr_count"] for k in (reg, big, build)}
    assert got == {reg: 119, big: 60, build: 36}, got


def test_isa_lint_of_the_track_kernels():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_chan_track.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 3 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
