"""CPU tier: the band activity detector (include/iqdemod.h: "Band activity") without a GPU - the mutation proof of the GPU
test's inputs (tests/detect_cases.py) on the numpy model (tests/detect_model.py), the model on the two synthetic stations
against where they were put, iqd_detect_offset_hz against Python's floor division, and the cross-compiled kernel's code
object."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def models(capi):
    """name -> (case, rows, det): every expected array is computed once"""
    out = {}
    for c in dc.cases(capi.channelizer_phasor_table()):
        rows, det = dm.detect(c.power, c.cfg)
        rows.setflags(write=False)
        det.setflags(write=False)
        out[c.name] = (c, rows, det)
    return out


def test_case_list_covers_what_the_kernel_can_get_wrong(models):
    cs = [c for c, _, _ in models.values()]
    assert {c.cfg.n_bins for c in cs} >= {64, 128, 256, 1024, 2048}
    assert {len(c.power) for c in cs} >= {1, 3, 65}
    assert {c.cfg.max_detections for c in cs} >= {1, 4} and any(c.cfg.max_detections == c.cfg.n_bins // 2 for c in cs)
    assert {c.cfg.bridge for c in cs} >= {0, 1, 5, 64} and {c.cfg.dc_guard for c in cs} >= {0, 1, 3}
    assert max(c.power.nbytes for c in cs) <= 65 * 128 * 4                 # 33 KiB: seconds on any machine


# Which cases must see which defect.  A defect not named for a case may still show there by chance (tail_kept shows
# wherever a row has fewer than K runs, centroid_round wherever a remainder reaches one half), so a case is held only to
# what it was planted for; what the others cannot see by construction:
#   rank_*, floor_zero, ge      only where a neighbouring rank differs, f = 0, or a bin equals T: the flat and duplicate rows
#   prod32                      only where f Q reaches 2^32 (N256-big; the saturated row too); no_sat only where
#                               (f Q) >> 8 reaches 2^32, which no row with a hot bin can have (nothing is above 2^32 - 1)
#   guard_*, peak_all_bins      only where d >= 1 and the bin next to the guard / under it is above T: the dc cases (a
#                               cold bin inside a run is at most T, below every hot bin, so only a guarded spike can be a
#                               peak that no hot bin is)
#   bridge_*                    only where a gap is exactly g or g + 1: the gaps cases
#   width_nhot, hot_bins_kept_only   only where a run is dropped or kept by its bridged width: N128-widths
#   peak_tie_high               only where a run has its largest value twice
#   sum32, ksum32               only where a sum reaches 2^32: N256-big (sum k p does in most runs of large bins too)
#   found_capped                only where n_found > K;  wrap only with hot bins within g of both ends
MUST_SEE = {
    "rank_low": ["N128-dup-rank"], "rank_high": ["N128-dup-rank"], "floor_zero": ["N64-flat"], "ge": ["N64-flat"],
    "prod32": ["N256-big", "N64-saturated"], "no_sat": ["N64-saturated"],
    "guard_le_low": ["N256-dc-d1", "N256-dc-d3"], "guard_le_high": ["N256-dc-d1", "N256-dc-d3"],
    "guard_in_sums": ["N256-dc-d1", "N256-dc-d3"],
    "bridge_low": ["N256-gaps-g0", "N256-gaps-g1", "N1024-gaps-g5", "N1024-gaps-g64"],
    "bridge_high": ["N256-gaps-g0", "N256-gaps-g1", "N1024-gaps-g5", "N1024-gaps-g64"],
    "width_nhot": ["N128-widths"], "peak_all_bins": ["N256-dc-d1", "N256-dc-d3"], "peak_tie_high": ["N64-peaks"],
    "sum32": ["N256-big"], "ksum32": ["N256-big", "N2048-seams"], "centroid_round": ["N128-random-65", "N1024-stations"],
    "found_capped": ["N64-alternate-K4", "N1024-gaps-g5", "N1024-seams-K1"],
    "tail_kept": ["N64-flat", "N2048-alternate", "N128-random-65"], "hot_bins_kept_only": ["N128-widths"],
    "wrap": ["N128-ends"],
}


def test_every_defect_is_seen_by_the_cases_planted_for_it(models):
    """The model with one defect switched on must change some entry of either output array on each case named for it."""
    assert sorted(MUST_SEE) == sorted(dm.DEFECTS)
    for defect, names in MUST_SEE.items():
        for name in names:
            c, rows, det = models[name]
            r2, d2 = dm.detect(c.power, c.cfg, defect)
            assert not (np.array_equal(rows, r2) and np.array_equal(det, d2)), (defect, name)


def test_model_outputs_hold_what_the_specification_implies(models):
    """on every case: a zeroed tail, records ascending and further apart than the bridge, widths of at least m, the
    centroid inside its run, every peak above the threshold, no more hot bins in runs than in the row"""
    for c, rows, det in models.values():
        assert rows.shape == (len(c.power),) and det.shape == (len(c.power), c.cfg.max_detections)
        for i in range(len(rows)):
            n = min(int(rows[i]["n_found"]), c.cfg.max_detections)
            assert not det[i, n:].view(np.uint8).any()
            d = det[i, :n]
            assert (d["first_bin"][1:] > d["last_bin"][:-1] + c.cfg.bridge + 1).all()      # separate, ascending
            assert (d["last_bin"] - d["first_bin"] + 1 >= c.cfg.min_width).all() and (d["n_hot"] >= 1).all()
            assert ((d["first_bin"] << 8) <= d["centroid_q8"]).all() and (d["centroid_q8"] < ((d["last_bin"] + 1) << 8)).all()
            assert (d["peak_power"] > rows[i]["threshold"]).all()
            assert d["n_hot"].sum() <= rows[i]["n_hot_bins"]


def test_planted_cases_are_what_they_claim(models):
    c, rows, det = models["N64-flat"]
    assert rows.tolist() == [(0, 1, 0, 0), (7, 7, 0, 0), (dm.M32, dm.M32, 0, 0)]
    c, rows, det = models["N128-dup-rank"]
    assert rows["floor"].tolist() == [100, 100, 100, 0x01000001, 0x0100ff00]
    assert [dm.detect(c.power, c.cfg, "rank_low")[0]["floor"][i] for i in (0, 3)] == [50, 0x01000000]      # the first duplicate
    assert dm.detect(c.power, c.cfg, "rank_high")[0]["floor"][1] == 3007                                     # the last one
    c, rows, det = models["N256-big"]
    assert (rows["floor"].astype(np.uint64) * c.cfg.ratio_q8 >= 2 ** 32).all() and (rows["threshold"] < 2 ** 28).all()
    assert det[0, 0]["sum_power"] == 7 * dm.M32 and det["sum_power"].max() > 2 ** 34
    assert (det[0, 1]["first_bin"], det[0, 1]["last_bin"]) == (60, 69)                # over the seam at 64
    c, rows, det = models["N64-saturated"]
    assert rows.tolist() == [(int(np.sort(c.power[0])[32]), dm.M32, 0, 0)] and c.power.max() == dm.M32
    for name in ("N64-alternate-K4", "N2048-alternate"):
        c, rows, det = models[name]
        assert rows["n_found"][0] == c.cfg.n_bins // 2 and (det[0]["first_bin"] == det[0]["last_bin"]).all()
    assert models["N64-alternate-K4"][1]["n_found"][0] > models["N64-alternate-K4"][0].cfg.max_detections
    c, rows, det = models["N2048-alternate"]
    assert det[1, 0]["first_bin"] == 0 and rows["n_found"][2] < c.cfg.max_detections
    for name in ("N256-gaps-g0", "N256-gaps-g1", "N1024-gaps-g5", "N1024-gaps-g64"):
        c, rows, det = models[name]
        g = c.cfg.bridge
        assert rows["n_found"].tolist() == [6, 6, 6] and rows["n_hot_bins"].tolist() == [8, 8, 8]           # g joins, g + 1 splits
        widths = (det["last_bin"].astype(int) - det["first_bin"] + 1)[:, :min(6, c.cfg.max_detections)]
        assert (widths[:, 0] == g + 2).all() and (widths[:, 1:3] == 1).all()
    c, rows, det = models["N128-ends"]
    assert rows["n_found"].tolist() == [2, 2] and det[:, 0]["first_bin"].tolist() == [0, 0]
    assert det[:, 1]["last_bin"].tolist() == [127, 127]
    c, rows, det = models["N2048-seams"]
    assert [(int(r["first_bin"]), int(r["last_bin"])) for r in det[0]] == [(57, 130), (250, 261), (1020, 1029), (1848, 2017)]
    assert (det[2, 0]["first_bin"], det[2, 0]["last_bin"], det[2, 0]["n_hot"]) == (63, 259, 5)             # whole cold words bridged
    assert (det[2, 1]["first_bin"], det[2, 1]["last_bin"]) == (400, 465) and rows["n_found"][2] == 2
    c, rows, det = models["N1024-seams-K1"]                                             # g = 1: the same bins, unbridged
    assert rows["n_found"].tolist() == [4, 4, 1] and (det[0, 0]["first_bin"], det[0, 0]["last_bin"]) == (57, 63)
    assert (det[2, 0]["first_bin"], det[2, 0]["last_bin"]) == (258, 259)
    c, rows, det = models["N256-dc-d1"]
    assert (det[0, 0]["first_bin"], det[0, 0]["last_bin"], det[0, 0]["n_hot"]) == (122, 134, 12) and det[0, 0]["peak_power"] < 9000
    assert rows["n_found"][2] == 0                                                      # the lone spike is guarded away
    assert models["N256-dc-d0"][2][0, 0]["peak_power"] == 4000000000 and models["N256-dc-d0"][2][0, 0]["peak_bin"] == 128
    c, rows, det = models["N128-widths"]
    assert [(int(r["first_bin"]), int(r["last_bin"]), int(r["n_hot"])) for r in det[0, :3]] == [(10, 13, 4), (62, 65, 2), (100, 103, 2)]
    assert rows[0]["n_found"] == 3 and rows[0]["n_hot_bins"] == 4 + 3 + 2 + 2 + 2
    c, rows, det = models["N64-peaks"]
    assert det[0, 0]["peak_bin"] == 21 and det[1, 0]["peak_bin"] == 0 and det[1, 1]["peak_bin"] == 61


def test_two_stations_are_found_where_they_were_put(models, capi):
    """The model on the spectrum model's rows of synth.wideband's two stations, with the README line's parameters: exactly
    two runs per block, each centred within one bin width of the station's true offset.  This is the model against a
    known truth, never the device against itself."""
    c, rows, det = models["N1024-stations"]
    assert c.cfg == dc.readme_cfg(1024) == dm.Cfg(1024, 512, 2048, 1, 8, 3, 16)
    assert rows["n_found"].tolist() == [2, 2]
    for b in range(2):
        for r, st in zip(det[b, :2], dc.STATIONS):
            hz = dm.offset_hz(1024, dc.RATE, r["centroid_q8"])
            assert hz == capi.detect_offset_hz(1024, dc.RATE, r["centroid_q8"])
            assert abs(hz - st["offset"]) <= dc.RATE / 1024, (b, hz, st["offset"])
            assert r["first_bin"] <= r["peak_bin"] <= r["last_bin"]


def test_offset_hz_is_pythons_floor_division(capi):
    L = capi._lib()
    hz = C.c_int64(7)
    rng = np.random.default_rng(21)
    for N in dm.N_SET:
        cents = [0, 1, 127, 128, 128 * N - 1, 128 * N, 128 * N + 1, 256 * N - 1] + rng.integers(0, 256 * N, 40).tolist()
        for rate in (1, 3, 250000, 1024000, 2048000, 2400000, 2 ** 32 - 1):
            for cq in cents:
                want = ((cq - 128 * N) * rate + 128 * N) // (256 * N)
                assert dm.offset_hz(N, rate, cq) == want
                assert L.iqd_detect_offset_hz(N, rate, cq, C.byref(hz)) == 0 and hz.value == want, (N, rate, cq)
        # the centre of bin k is k rate / N from the band's lower edge: the centre of bin N / 2 is offset 0, bin 0's -rate / 2
        assert capi.detect_offset_hz(N, 2048000, 256 * (N // 2)) == 0
        assert capi.detect_offset_hz(N, 2048000, 0) == -1024000
        assert 1024000 - 2048000 // N <= capi.detect_offset_hz(N, 2048000, 256 * N - 1) < 1024000
    assert capi.detect_offset_hz(64, 1000, 8000) == -12 and -183808 / 16384 > -11.3                       # floor, not truncation
    hz = C.c_int64(7)
    for bad in ((0, 1000, 0), (100, 1000, 0), (4096, 1000, 0), (64, 0, 0), (64, 1000, 256 * 64), (2048, 1000, 2 ** 32 - 1)):
        assert L.iqd_detect_offset_hz(*bad, C.byref(hz)) == -1 and hz.value == 7, bad
        with pytest.raises(capi.IqdError):
            capi.detect_offset_hz(*bad)
    assert L.iqd_detect_offset_hz(64, 1000, 0, None) == -1


def test_structures_are_the_headers(capi):
    assert capi.DETECT_ROW == dm.ROW_DTYPE and capi.DETECTION == dm.DET_DTYPE
    assert C.sizeof(capi.DetectConfig) == 32 and capi.DETECT_ROW.itemsize == 16 and capi.DETECTION.itemsize == 32
    assert [capi.DETECTION.fields[n][1] for n in capi.DETECTION.names] == [0, 4, 8, 12, 16, 24, 28]


@pytest.fixture(scope="module")
def code_object():
    """iqd_detect.hip cross-compiled for gfx950 (device only, the library's flags): {kernel: metadata}, the text"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "iqd_detect.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
               os.path.join(csrc, "iqd_detect.hip")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(asm).read()
        for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
            kernel = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[kernel] = {k: int(v) for k, v in re.findall(
                r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\d+)", blk)}
    return meta, text


def test_code_object(code_object):
    meta, text = code_object
    assert sorted(meta) == ["_ZN3iqd10det_kernelENS_9DetLaunchE"]
    m = meta["_ZN3iqd10det_kernelENS_9DetLaunchE"]
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert m["group_segment_fixed_size"] == 4 * (8192 + 1024), m         # per wave: the row and 256 counters
    assert m["vgpr_count"] == 70, m
    assert "global_atomic" not in text and "buffer_atomic" not in text and "flat_atomic" not in text
    assert text.count("ds_add_u32") == 4 * 32                            # the histogram: LDS atomics only, 32 values a lane and pass


def test_isa_lint_of_the_detector_kernel():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_detect.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 1 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
