"""CPU tier: the band track measurements (include/iqdemod.h: "Band track measurements") without a GPU - the mutation proof of
the GPU test's inputs (tests/measure_cases.py) on the direct-sum model (tests/measure_model.py), what the model's outputs must
hold, the header's records against the binding's, the default thresholds on a capture of an AM, a narrow FM and a wide FM
station through the chained models, and the cross-compiled kernel's code object."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import detect_cases as dc
from tests import detect_model as dm
from tests import measure_cases as mc
from tests import measure_model as mm
from tests import spectrum_model as sm
from tests import track_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def models():
    """name -> (case, meas): every expected array is computed once"""
    out = {}
    for c in mc.cases():
        meas = mc.model(c)
        meas.setflags(write=False)
        out[c.name] = (c, meas)
    return out


def test_case_list_covers_what_the_kernel_can_get_wrong(models):
    cs = [c for c, _ in models.values()]
    assert [c.name for c in cs] == mc.NAMES
    assert {c.cfg.n_bins for c in cs} >= {64, 128, 256, 512, 1024, 2048} and {c.cfg.n_slots for c in cs} >= {1, 4, 5, 8, 64}
    assert {c.cfg.n_sources for c in cs} >= {1, 3} and {c.n_blocks for c in cs} >= {1, 3}
    assert {c.cfg.obw_tail_q16 for c in cs} >= {0, 32767} and {c.cfg.carrier_half for c in cs} >= {0, 8}
    assert {c.cfg.margin for c in cs} >= {0, 64} and {c.cfg.dc_guard for c in cs} >= {0, 1, 3}
    spans = set()
    for c, meas in models.values():
        live = c.slots[c.slots["state"] != 0]
        spans |= set((live["last_bin"].astype(int) - live["first_bin"] + 1).tolist())
    assert spans >= {1, 63, 64, 65, 128, 129, 2048}
    kinds = np.concatenate([np.stack([c.slots["state"].ravel(), c.slots["track_id"].ravel() != 0], 1) for c, _ in models.values()])
    assert {tuple(k) for k in kinds.tolist()} == {(0, 0), (0, 1), (1, 1), (2, 1)}      # free, closing, tentative, active
    flags = np.concatenate([m["flags"].ravel() for _, m in models.values()])
    hints = np.concatenate([m["hint"].ravel() for _, m in models.values()])
    assert set(flags.tolist()) == {0, mm.F_EMPTY, mm.F_WEAK} and set(hints.tolist()) == {0, 1, 2, 3}
    assert max(int(m["sum_excess"].max()) for _, m in models.values()) == 2048 * (2 ** 32 - 1)       # the largest sum there is
    assert max(c.power.nbytes for c in cs) <= 3 * 3 * 2048 * 4


# Which cases must see which defect.  A defect not named for a case may still show there (floor_kept, centroid_rel and
# margin_dropped show almost everywhere), so a case is held only to what it was planted for; what the others cannot see by
# construction:
#   floor_ge                only where a bin of a window is exactly at the floor and not guarded
#   guard_counted           only where a window reaches into the guard and a guard bin is over the floor
#   no_clip_lo, no_clip_hi  only where first_bin < m (last_bin + m > N - 1) in a row that has another row of the source before
#                           (behind) it with excess there; the first row of a source reads nothing before it
#   margin_dropped          only at m > 0 with excess in the margin;  beta_total only at beta >= 2
#   obw_lo_ge, obw_hi_ge    only where 65536 L == beta E (R likewise) for some bin: N64-obw-edge, and beta = 0 (where L = 0 on
#                           the bins under the floor at the window's ends)
#   peak_high               only where the maximum is taken twice;  carrier_unclipped only where peak_bin - c < lo (or
#                           peak_bin + c > hi) with excess there
#   closing_measured        only with a closing slot whose window has excess;  empty_kept only with E = 0
#   weak_hinted             only with 0 < E < min_sum;  hint_order only where a record is wide and has its carrier
#   floor_source0           only with two sources whose floors differ;  power_prev_block only from the second block on
MUST_SEE = {
    "floor_kept": ["N64-S1-basics", "N64-minsum", "N64-obw-edge"], "floor_ge": ["N64-S1-basics", "N64-minsum"],
    "guard_counted": ["N64-guard", "N64-empty"], "no_clip_lo": ["N64-edges", "N128-sources3"],
    "no_clip_hi": ["N64-edges", "N128-sources3"], "margin_dropped": ["N64-S1-basics", "N64-edges", "N64-guard", "N2048-saturated"],
    "obw_lo_ge": ["N64-obw-edge", "N64-beta0"], "obw_hi_ge": ["N64-obw-edge", "N64-beta0"],
    "beta_total": ["N64-obw-edge", "N64-beta-max", "N2048-saturated"], "peak_high": ["N64-peak-ties", "N64-saturated", "N2048-saturated"],
    "carrier_unclipped": ["N64-carrier-c8-edge", "N2048-saturated"], "centroid_rel": ["N64-S1-basics", "N64-single-bin", "N2048-S64"],
    "closing_measured": ["N64-states-overlap", "N2048-S64"], "empty_kept": ["N64-empty"], "weak_hinted": ["N64-minsum", "N64-hints"],
    "hint_order": ["N64-hints"], "floor_source0": ["N128-sources3", "N512-random"],
    "power_prev_block": ["N64-S1-basics", "N64-edges", "N128-sources3", "N1024-random", "N2048-S64"],
}


def test_every_defect_is_seen_by_the_cases_planted_for_it(models):
    """The model with one defect switched on must change some entry of the output on each case named for it."""
    assert sorted(MUST_SEE) == sorted(mm.DEFECTS)
    for defect, names in MUST_SEE.items():
        for name in names:
            c, meas = models[name]
            assert not np.array_equal(mc.model(c, defect), meas), (defect, name)


def test_model_outputs_hold_what_the_specification_implies(models):
    """(the model itself asserts the header's bounds on every entry it computes)"""
    for c, meas in models.values():
        cf = c.cfg
        assert meas.shape == c.slots.shape
        off = meas[c.slots["state"] == 0]
        assert not off.view(np.uint8).any()                                    # free and closing slots: 32 zero bytes
        on, sl = meas[c.slots["state"] != 0], c.slots[c.slots["state"] != 0]
        assert np.array_equal(on["track_id"], sl["track_id"]) and on["track_id"].all()
        empty = on[on["flags"] == mm.F_EMPTY]
        z = empty.copy()
        z["track_id"], z["flags"] = 0, 0
        assert not z.view(np.uint8).any()
        full = on[on["flags"] != mm.F_EMPTY]
        assert (full["obw_lo"] <= full["obw_hi"]).all() and (full["carrier_q8"] <= 256).all() and (full["sum_excess"] > 0).all()
        assert ((full["flags"] == mm.F_WEAK) == (full["sum_excess"] < cf.min_sum)).all()
        assert (full["hint"][full["flags"] == mm.F_WEAK] == 0).all() and (full["hint"][full["flags"] == 0] != 0).all()
        assert (full["peak_excess"] <= full["sum_excess"]).all() and (full["n_over"] >= 1).all()


def test_planted_entries_are_what_was_planted(models):
    """the OBW edge case by hand, the min_sum pair, the hints, the single bins"""
    _, m = models["N64-obw-edge"]
    assert (m[0, 0, 0]["obw_lo"], m[0, 0, 0]["obw_hi"], m[0, 0, 0]["sum_excess"]) == (21, 22, 400)
    _, m = models["N64-minsum"]
    assert m[0, 0]["sum_excess"].tolist() == [5000, 4999] and m[0, 0]["flags"].tolist() == [0, mm.F_WEAK]
    _, m = models["N64-hints"]
    assert m[0, 0]["hint"].tolist() == [mm.CARRIER, mm.NARROW, mm.WIDE, mm.WIDE] and m[0, 1, 0]["hint"] == mm.NONE
    assert m[0, 0, 3]["carrier_q8"] >= 128
    c, m = models["N64-single-bin"]
    for s, k in ((0, 40), (1, 63), (2, 0)):
        x = m[0, 0, s]
        assert (x["obw_lo"], x["obw_hi"], x["peak_bin"], x["centroid_q8"], x["carrier_q8"], x["n_over"]) == (k, k, k, 256 * k, 256, 1)
    _, m = models["N64-peak-ties"]
    assert m[0, 0]["peak_bin"].tolist() == [20, 44]
    _, m = models["N2048-saturated"]
    assert m[0, 0, 0]["sum_excess"] == 2048 * (2 ** 32 - 1) and m[0, 0, 0]["n_over"] == 2048


def test_structures_are_the_headers(capi):
    assert capi.TRACK_MEASURE == mm.MEAS_DTYPE and capi.TRACK_MEASURE.itemsize == 32 and C.sizeof(capi.MeasureConfig) == 48
    assert [capi.TRACK_MEASURE.fields[n][1] for n in capi.TRACK_MEASURE.names] == [0, 4, 6, 8, 10, 11, 12, 16, 20, 22, 24]
    header = open(os.path.join(ROOT, "include", "iqdemod.h")).read()
    body = re.search(r"typedef struct iqd_track_measure \{(.*?)\} iqd_track_measure;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == list(capi.TRACK_MEASURE.names)
    body = re.search(r"typedef struct iqd_measure_config \{(.*?)\} iqd_measure_config;", header, re.S).group(1)
    fields = re.findall(r"uint32_t\s+(\w+)", body)
    assert fields == [f[0] for f in capi.MeasureConfig._fields_]
    for name, value in (("IQD_MEASURE_F_EMPTY", mm.F_EMPTY), ("IQD_MEASURE_F_WEAK", mm.F_WEAK), ("IQD_HINT_NONE", mm.NONE),
                        ("IQD_HINT_CARRIER", mm.CARRIER), ("IQD_HINT_NARROW", mm.NARROW), ("IQD_HINT_WIDE", mm.WIDE)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert (capi.MEASURE_F_EMPTY, capi.MEASURE_F_WEAK) == (mm.F_EMPTY, mm.F_WEAK)
    assert (capi.HINT_NONE, capi.HINT_CARRIER, capi.HINT_NARROW, capi.HINT_WIDE) == (0, 1, 2, 3)
    for name in ("iqd_measure_create", "iqd_measure_destroy", "iqd_measure_run_device", "iqd_measure_run"):
        assert name in capi.EXPORTS and getattr(capi._lib(), name)


def three_station_chain(capi):
    """the three-station capture through the spectrum, detector and tracker models (README's parameters) and the measurement
    model under the default thresholds: (slots, meas), [1, blocks, S]"""
    k = mc.THREE
    N, F, nb, S = k["N"], k["F"], k["blocks"], k["S"]
    power = sm.spectrum(mc.three_wide(), "u8", N, F, None, capi.channelizer_phasor_table())
    rows, det = dm.detect(power.reshape(-1, N), dc.readme_cfg(N))
    slots, _ = tm.Tracker(tm.Cfg(1, N, 16, S, 512, 3, 2, 64, 0, capi.track_default_edges(N))).run(rows.reshape(1, nb), det.reshape(1, nb, 16))
    d = capi.measure_defaults(N)
    cfg = mm.Cfg(1, N, S, 1, d["margin"], d["obw_tail_q16"], d["carrier_half"], d["min_sum"], d["carrier_min_q8"], d["wide_bins"])
    return slots, mm.measure(power.reshape(1, nb, N), rows.reshape(1, nb), slots, cfg)


def test_default_thresholds_name_an_am_a_narrow_fm_and_a_wide_fm_station(capi):
    """in every block in which the three tracks are live the hints are CARRIER, NARROW, WIDE, and the measurements lie where
    DESIGN 4.15 records them: well away from the thresholds on both sides"""
    slots, meas = three_station_chain(capi)
    N = mc.THREE["N"]
    d = capi.measure_defaults(N)
    seen = 0
    for b in range(mc.THREE["blocks"]):
        live = [(t, x) for t, x in zip(slots[0, b], meas[0, b]) if t["state"] != 0]
        assert len(live) == 3
        for t, x in live:
            hz = dm.offset_hz(N, mc.RATE, int(x["centroid_q8"]))
            st = min(mc.THREE_STATIONS, key=lambda s: abs(s["offset"] - hz))
            assert abs(st["offset"] - hz) <= 4 * mc.RATE / N and x["flags"] == 0
            assert x["hint"] == mc.THREE_HINTS[st["mode"]], (b, st["mode"], x)
            width, carrier = int(x["obw_hi"]) - int(x["obw_lo"]) + 1, int(x["carrier_q8"])
            lo_c, hi_c, lo_w, hi_w = {"am": (215, 256, 5, 12), "fm": (60, 110, 12, 20), "wbfm": (5, 30, 150, 175)}[st["mode"]]
            assert lo_c <= carrier <= hi_c and lo_w <= width <= hi_w, (b, st["mode"], carrier, width)
            seen += 1
    assert seen == 3 * mc.THREE["blocks"]
    assert 110 < d["carrier_min_q8"] < 215 and 20 < d["wide_bins"] < 150


KERNEL = "_ZN3iqd10msr_kernelENS_9MsrLaunchE"


@pytest.fixture(scope="module")
def code_object():
    """iqd_measure.hip cross-compiled for gfx950 (device only, the library's flags): {kernel: metadata}, the text"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "iqd_measure.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
               os.path.join(csrc, "iqd_measure.hip")]
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
    assert m["group_segment_fixed_size"] == 2 * (8 * 2049 + 8) + 2 * 4 * 8, m # the two prefix arrays (each padded to 16 bytes) and the waves' totals
    assert m["vgpr_count"] <= 80, m                                           # DESIGN 4.15 records the figure
    assert "global_atomic" not in text and "buffer_atomic" not in text and "flat_atomic" not in text and "ds_add" not in text
    assert text.count("global_store_dwordx4") == 2                            # a record's two halves, nothing else is stored
    assert "global_load_dwordx4" in text


def test_isa_lint_of_the_measure_kernel():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_measure.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 1 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
