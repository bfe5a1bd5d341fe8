"""CPU tier: the band activity tracker (include/iqdemod.h: "Band tracks") without a GPU - the mutation proof of the GPU
test's inputs (tests/track_cases.py) on the Python-int model (tests/track_model.py), the split-call property on the model,
iqd_track_phase_inc against the formula and against channelizer_tuning, the chained case against where and when its
stations were put, and the cross-compiled kernel's code object."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import detect_model as dm
from tests import track_cases as tc
from tests import track_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def models(capi):
    """name -> (case, slots, blocks): every expected array is computed once"""
    out = {}
    for c in tc.cases(capi.channelizer_phasor_table()):
        slots, blocks = tc.model(c)
        slots.setflags(write=False)
        blocks.setflags(write=False)
        out[c.name] = (c, slots, blocks)
    return out


def test_case_list_covers_what_the_kernel_can_get_wrong(models):
    cs = [c for c, _, _ in models.values()]
    assert [c.name for c in cs] == tc.NAMES
    assert {c.cfg.n_bins for c in cs} >= {64, 2048} and {c.cfg.n_slots for c in cs} >= {1, 3, 64}
    assert {c.cfg.max_detections for c in cs} >= {1, 4, 16, 128} and {c.cfg.n_sources for c in cs} >= {1, 3}
    assert {c.cfg.hold_blocks for c in cs} >= {0, 1, 2} and {c.cfg.open_hits for c in cs} >= {1, 2, 3, 255}
    assert {c.cfg.alpha_q8 for c in cs} >= {1, 64, 256}
    assert min(c.n_blocks for c in cs) <= 2 and sorted(c.n_blocks for c in cs)[-2:] == [24, 300]
    assert any(int(c.rows["n_found"].max()) > c.cfg.max_detections for c in cs)
    assert max(c.det.nbytes for c in cs) <= 4 * 128 * 32 and max(s.nbytes for _, s, _ in models.values()) <= 300 * 32


# Which cases must see which defect.  A defect not named for a case may still show there (age_alloc, flags_kept and
# alloc_high show almost everywhere), so a case is held only to what it was planted for; what the others cannot see by
# construction:
#   tie_high, first_in_gate   only where two live slots are in one detection's gate: N64-ties, N64-nearest
#   gate_lt                   only where a distance is exactly G: N64-gate, N64-ties (N2048-edges-bias: G = 0)
#   match_twice               only where two detections of a block are in one slot's gate and in no other's
#   shift_trunc               only where (c - centre) A is negative and no multiple of 256;  alpha256 only at A = 256
#   hits_unsat                only past 255 blocks;  open_late / close_ge / tentative_survives need an open, a close at
#                             B >= 1 (at B = 0 both rules close at the first miss), a tentative miss
#   realloc_same_block        only where a detection is unmatched in a block that frees or closes a slot and leaves no other
#   closed_kept               only where the slot of a closed record is not allocated in the very next block
#   shared_id                 only with two sources that both allocate;  no_carry, reset_keeps_id only with two calls, a reset
#   read_past_d               only where a row has fewer than K records and the rest is not what a free slot would ignore;
#                             found_over_k only where n_found > K
#   inc_sign                  only below the centre;  shift_2048 only at N = 2048;  bias_nowrap only where the sum passes 2^32
#   class_last                only where a track has been wider than it is;  unplaced_zero only where a detection is unplaced
#   updated_centres           alone it cannot be seen on any input at all: the centre that a match moves belongs to a slot
#                             that is matched, and a matched slot is not considered again in the block.  It is seen together
#                             with match_twice, where the rule is what decides (test_updated_centres_*).
MUST_SEE = {
    "tie_high": ["N64-ties"], "gate_lt": ["N64-gate", "N64-ties"], "first_in_gate": ["N64-nearest"],
    "match_twice": ["N64-S3-life"], "updated_centres": [], "shift_trunc": ["N64-S3-life", "N64-A1", "N256-chained"],
    "alpha256": ["N64-A256", "N64-ties"], "hits_unsat": ["N64-hits-300"],
    "open_late": ["N64-S3-life", "N64-B0-H1", "N64-hits-300", "N256-chained"],
    "close_ge": ["N64-S3-life", "N64-close-and-arrive", "N256-chained"], "tentative_survives": ["N64-S3-life", "N64-close-and-arrive"],
    "realloc_same_block": ["N64-close-and-arrive", "N2048-K128-S64"], "alloc_high": ["N64-S3-life", "N64-full-S3", "N2048-K128-S64"],
    "closed_kept": ["N64-B0-H1", "N256-chained"], "flags_kept": ["N64-S3-life", "N64-full-S1"],
    "age_alloc": ["N64-S3-life", "N64-full-S1"], "shared_id": ["N64-sources3", "N2048-edges-bias"],
    "no_carry": ["N64-S3-split-reset", "N64-sources3"], "reset_keeps_id": ["N64-S3-split-reset"],
    "read_past_d": ["N64-S3-life", "N2048-K128-S64"], "found_over_k": ["N64-found-over-K1", "N64-found-over-K4"],
    "inc_sign": ["N64-S3-life", "N2048-edges-bias"], "shift_2048": ["N2048-edges-bias", "N2048-K128-S64"],
    "bias_nowrap": ["N2048-edges-bias"], "class_last": ["N64-widths"],
    "unplaced_zero": ["N64-full-S1", "N64-full-S3", "N64-close-and-arrive", "N2048-K128-S64"],
}


def _differs(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


def test_every_defect_is_seen_by_the_cases_planted_for_it(models):
    """The model with one defect switched on must change some entry of either output array on each case named for it."""
    assert sorted(MUST_SEE) == sorted(tm.DEFECTS)
    for defect, names in MUST_SEE.items():
        for name in names:
            c, slots, blocks = models[name]
            assert _differs(tc.model(c, defect), (slots, blocks)), (defect, name)


def test_updated_centres_shows_only_where_a_slot_can_be_matched_twice(models):
    """alone the switch changes nothing on any case (see MUST_SEE); with match_twice it decides where the second detection of a small case goes"""
    for c, slots, blocks in models.values():
        assert not _differs(tc.model(c, "updated_centres"), (slots, blocks)), c.name
    twice = tc.Case("twice", tc.cfg(S=2, G=600, H=1, A=256), {(0, 0): [tc.d(20, 0), tc.d(30, 0)], (0, 1): [tc.d(21, 0), tc.d(23, 0)]}, 2)
    # slot 0 at 5120: detection 0 (5376) matches it; detection 1 (5888) is 768 away from the old centre (a new track) and
    # 512 from the moved one (a second match of slot 0)
    assert _differs(tc.model(twice, ("match_twice", "updated_centres")), tc.model(twice, "match_twice"))
    assert not _differs(tc.model(twice, "match_twice"), tc.model(twice))


def test_split_calls_give_what_one_call_gives(models):
    """on the model, every case in one call, block by block, and cut at every third block"""
    for c, slots, blocks in models.values():
        if any(op[0] == "reset" for op in c.calls) or c.n_blocks > 40:
            continue
        for step in (1, 3):
            t = tm.Tracker(c.cfg)
            got = [t.run(c.rows[:, b:b + step], c.det[:, b:b + step]) for b in range(0, c.n_blocks, step)]
            assert np.array_equal(np.concatenate([g[0] for g in got], axis=1), slots), (c.name, step)
            assert np.array_equal(np.concatenate([g[1] for g in got], axis=1), blocks), (c.name, step)
            for j in range(c.cfg.n_sources):
                assert np.array_equal(t.state(j), slots[j, -1])


def test_model_outputs_hold_what_the_specification_implies(models):
    for c, slots, blocks in models.values():
        cf = c.cfg
        assert slots.shape == (cf.n_sources, c.n_blocks, cf.n_slots) and blocks.shape == (cf.n_sources, c.n_blocks)
        free = slots[(slots["track_id"] == 0)]
        assert not free.view(np.uint8).any()                                   # a free slot is all-zero bytes
        live = slots[slots["track_id"] != 0]
        assert (live["centre_q8"] < 256 * cf.n_bins).all() and (live["hits"] >= 1).all() and (live["misses"] <= cf.hold_blocks + 1).all()
        assert ((live["state"] == 0) == ((live["flags"] & 8) != 0)).all()      # a record with an id and state 0 is closing
        assert (blocks["n_active"] == (slots["state"] == 2).sum(axis=2)).all() and (blocks["n_tentative"] == (slots["state"] == 1).sum(axis=2)).all()
        for j in range(0 if any(op[0] == "reset" for op in c.calls) else cf.n_sources):   # ids: 1, 2, ... as they appear
            ids = slots[j]["track_id"][(slots[j]["flags"] & 2) != 0]
            assert ids.tolist() == list(range(1, len(ids) + 1))


def test_phase_inc_is_the_formula(capi):
    L = capi._lib()
    inc = C.c_uint32(7)
    rng = np.random.default_rng(23)
    for N in tm.N_SET:
        sh = 24 - (N.bit_length() - 1)
        cents = [0, 1, 128 * N - 1, 128 * N, 128 * N + 1, 256 * N - 1] + rng.integers(0, 256 * N, 40).tolist()
        for bias in (0, 1, 0x40000000, 0xC0000001, 2 ** 32 - 1):
            for cq in cents:
                want = (((cq - 128 * N) << sh) + bias) % 2 ** 32
                assert tm.phase_inc(N, cq, bias) == want
                assert L.iqd_track_phase_inc(N, cq, bias, C.byref(inc)) == 0 and inc.value == want, (N, cq, bias)
        # both ends of the range: bin 0 is -1/2 of the wide rate, the centre 0, the last 1/256 bin one step under +1/2
        assert capi.track_phase_inc(N, 0) == 0x80000000 and capi.track_phase_inc(N, 128 * N) == 0
        assert capi.track_phase_inc(N, 256 * N - 1) == 0x80000000 - (1 << sh) and capi.track_phase_inc(N, 128 * N - 1) == 2 ** 32 - (1 << sh)
    for bad in ((0, 0, 0), (100, 0, 0), (4096, 0, 0), (64, 256 * 64, 0), (2048, 2 ** 32 - 1, 0)):
        inc = C.c_uint32(7)
        assert L.iqd_track_phase_inc(*bad, C.byref(inc)) == -1 and inc.value == 7, bad
        with pytest.raises(capi.IqdError):
            capi.track_phase_inc(*bad)
    assert L.iqd_track_phase_inc(64, 0, 0, None) == -1


def test_phase_inc_is_the_tuning_of_offset_hz(capi):
    """against channelizer_tuning(M = 8, rotation 0) of detect_offset_hz: the two may differ by the increment of 1 Hz,
    ceil(2^32 / rate), plus 1 - offset_hz rounds to whole Hz first"""
    rate = tc.RATE
    bound = -(-2 ** 32 // rate) + 1
    rng = np.random.default_rng(24)
    seen = 0
    for N in (64, 256, 2048):
        for cq in [0, 1, 128 * N - 1, 128 * N, 128 * N + 1, 256 * N - 1] + rng.integers(0, 256 * N, 30).tolist():
            hz = capi.detect_offset_hz(N, rate, cq)
            tuned = capi.channelizer_tuning(8, 100000000, 100000000 + hz, 0)
            if tuned is None:                                              # (the tuning refuses the band's outermost part)
                assert abs(hz) > 0.4 * rate
                continue
            seen += 1
            diff = (capi.track_phase_inc(N, cq) - tuned + 2 ** 31) % 2 ** 32 - 2 ** 31
            assert abs(diff) <= bound, (N, cq, hz, diff, bound)
    assert seen >= 3 * 24


def test_the_chained_case_is_held_to_where_its_stations_were_put(models):
    """one run in blocks 0-5 and 15-23, two in 6-14; exactly two ids ever; the second track is tentative in blocks 6-7, opens
    in block 8, is last matched in block 14 and closes in block 17; active centres within one bin width of -700 and +250 kHz"""
    c, slots, blocks = models["N256-chained"]
    assert c.rows["n_found"][0].tolist() == [1] * 6 + [2] * 9 + [1] * 9
    s = slots[0]
    assert sorted(set(s["track_id"].ravel().tolist())) == [0, 1, 2]
    second = [s[b][s[b]["track_id"] == 2] for b in range(24)]
    assert [len(x) for x in second] == [0] * 6 + [1] * 12 + [0] * 6
    assert [int(x["state"][0]) for x in second[6:18]] == [1, 1] + [2] * 9 + [0]
    assert [b for b in range(6, 18) if second[b]["flags"][0] & 4] == [8] and [b for b in range(6, 18) if second[b]["flags"][0] & 8] == [17]
    assert max(b for b in range(6, 18) if second[b]["flags"][0] & 1) == 14
    assert blocks[0]["n_opened_closed"].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 1] + [0] * 8 + [1 << 16] + [0] * 6
    assert not blocks[0]["n_unplaced"].any()
    for b in range(24):
        for x in s[b][s[b]["state"] == 2]:
            want = {1: -700e3, 2: 250e3}[int(x["track_id"])]
            assert abs(dm.offset_hz(256, tc.RATE, int(x["centre_q8"])) - want) <= tc.RATE / 256
            assert x["phase_inc"] == tm.phase_inc(256, int(x["centre_q8"]), 0)


def test_structures_are_the_headers(capi):
    assert capi.TRACK_SLOT == tm.SLOT_DTYPE and capi.TRACK_BLOCK == tm.BLOCK_DTYPE
    assert C.sizeof(capi.TrackConfig) == 64 and capi.TRACK_SLOT.itemsize == 32 and capi.TRACK_BLOCK.itemsize == 16
    assert [capi.TRACK_SLOT.fields[n][1] for n in capi.TRACK_SLOT.names] == [0, 4, 5, 6, 7, 8, 10, 12, 16, 20, 22, 24, 28]
    assert capi.track_default_edges(64) == tc.cfg().class_edge


KERNEL = "_ZN3iqd10trk_kernelENS_9TrkLaunchE"


@pytest.fixture(scope="module")
def code_object():
    """iqd_track.hip cross-compiled for gfx950 (device only, the library's flags): {kernel: metadata}, the text"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "iqd_track.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
               os.path.join(csrc, "iqd_track.hip")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(asm).read()
        for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
            kernel = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[kernel] = {k: int(v) for k, v in re.findall(
                r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\d+)", blk)}
    return meta, text


def test_code_object(code_object):
    meta, text = code_object
    assert sorted(meta) == [KERNEL]
    m = meta[KERNEL]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == 0, m                          # no LDS
    assert m["vgpr_count"] <= 64, m                                       # DESIGN 4.14 records the figure
    assert "global_atomic" not in text and "buffer_atomic" not in text and "flat_atomic" not in text
    assert "s_barrier" not in text
    assert text.count("global_store_dwordx4") >= 5                        # two per slot record and state record, one per block record


def test_isa_lint_of_the_tracker_kernel():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_track.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 1 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
