"""GPU (MI355X): the band activity detector (include/iqdemod.h: "Band activity") exactly equal to the numpy model
(tests/detect_model.py) on the inputs of tests/detect_cases.py (which tests/test_detect_host.py holds to the mutation
proof) - both output arrays in full, in host and device form - beside a Spectrum on one engine, chained behind
Spectrum.run_device on one stream, its refusals, and through the iqdemod_spectrum tool.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import detect_cases as dc
from tests import detect_model as dm
from tests import spectrum_model as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_spectrum")


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def cases(P):
    return {c.name: c for c in dc.cases(P)}


@pytest.fixture(scope="module")
def wants(cases):
    """name -> the model's two arrays, computed once and shared"""
    out = {}

    def get(name):
        if name not in out:
            out[name] = dm.detect(cases[name].power, cases[name].cfg)
            for a in out[name]:
                a.setflags(write=False)
        return out[name]
    return get


def _same(got, want):
    """both arrays, every byte"""
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (len(bad), bad[:8], g[tuple(bad[0])], w[tuple(bad[0])])
        assert g.tobytes() == w.tobytes()


def _detector(capi, eng, cfg):
    return capi.Detector(eng, cfg.n_bins, cfg.floor_rank, cfg.ratio_q8, cfg.dc_guard, cfg.bridge, cfg.min_width, cfg.max_detections)


def _download(capi, eng, d_rows, d_det, n_rows, K):
    rows = eng.dev_download(d_rows, 16 * n_rows).view(capi.DETECT_ROW)
    det = eng.dev_download(d_det, 32 * n_rows * K).view(capi.DETECTION).reshape(n_rows, K)
    return rows, det


@pytest.mark.parametrize("name", dc.NAMES)
def test_equal_to_the_model(capi, cases, wants, name):
    """the host form; the device form into buffers full of stale bytes (every record is written, the tail as zeros); a
    second device call into the same buffers (no state from call to call)"""
    c, want = cases[name], wants(name)
    n_rows, K = len(c.power), c.cfg.max_detections
    eng = capi.Engine(1)
    d = _detector(capi, eng, c.cfg)
    _same(d.run(c.power), want)
    d_in, d_rows, d_det = eng.dev_alloc(c.power.nbytes), eng.dev_alloc(16 * n_rows), eng.dev_alloc(32 * n_rows * K)
    eng.dev_upload(d_in, c.power.view(np.uint8))
    eng.dev_upload(d_rows, np.full(16 * n_rows, dm.STALE, np.uint8))
    eng.dev_upload(d_det, np.full(32 * n_rows * K, dm.STALE, np.uint8))
    for _ in range(2):
        d.run_device(d_in, n_rows, d_rows, d_det)
        eng.synchronize()
        _same(_download(capi, eng, d_rows, d_det, n_rows, K), want)
    assert np.array_equal(eng.dev_download(d_in, c.power.nbytes), c.power.view(np.uint8).ravel())      # the rows are only read
    for p in (d_in, d_rows, d_det):
        eng.dev_free(p)
    d.close()
    eng.close()


def test_beside_a_spectrum_on_one_engine(capi, P, cases, wants):
    """One engine: a Spectrum and two Detectors of different shapes, called in turn; each gives what it gives alone."""
    rng = np.random.default_rng(91)
    wide = rng.integers(0, 256, (1, 2 * 64 * 4 * 3), dtype=np.uint8)
    eng = capi.Engine(1)
    s = capi.Spectrum(eng, 64)
    a, b = cases["N64-peaks"], cases["N2048-seams"]
    da, db = _detector(capi, eng, a.cfg), _detector(capi, eng, b.cfg)
    power = sm.spectrum(wide, "u8", 64, 4, None, P)
    for _ in range(2):
        _same(da.run(a.power), wants(a.name))
        assert np.array_equal(s.run(wide, 4), power)
        _same(db.run(b.power), wants(b.name))
    # and a detector on what the spectrum just gave (three rows of noise)
    _same(da.run(s.run(wide, 4)), dm.detect(power[0], a.cfg))
    for o in (da, db, s):
        o.close()
    eng.close()


@pytest.mark.parametrize("fmt", ["u8", "s8"])
def test_chained_behind_the_spectrum_on_one_stream(capi, P, fmt):
    """Spectrum.run_device then Detector.run_device, queued back to back with no synchronise between them: the detector
    reads the rows the spectrum writes.  Against the detector's model fed the spectrum model's rows; three sources."""
    from rtlsdrdiags_amd import synth
    N, F, blocks, n_src = 1024, 8, 2, 3
    u8 = np.stack([synth.wideband(N * F * blocks, float(dc.RATE), dc.STATIONS, seed=31 + i) for i in range(n_src)])
    u8[2] = np.roll(u8[2], 2 * 5)
    wide = np.ascontiguousarray(u8 if fmt == "u8" else (u8 ^ 0x80).view(np.int8))
    cfg = dc.readme_cfg(N)
    power = sm.spectrum(wide, fmt, N, F, None, P)
    want = dm.detect(power.reshape(-1, N), cfg)
    assert want[0]["n_found"].tolist() == [2] * (n_src * blocks)
    eng = capi.Engine(1)
    s = capi.Spectrum(eng, N, n_sources=n_src, sample_format=fmt)
    d = capi.Detector(eng, N)                                             # the defaults are the README line's
    n_rows, K = n_src * blocks, cfg.max_detections
    d_in, d_pow = eng.dev_alloc(wide.nbytes), eng.dev_alloc(power.nbytes)
    d_rows, d_det = eng.dev_alloc(16 * n_rows), eng.dev_alloc(32 * n_rows * K)
    eng.dev_upload(d_in, wide.view(np.uint8))
    eng.dev_upload(d_pow, np.full(power.nbytes, dm.STALE, np.uint8))      # rows the detector must not see
    launches = eng.stats()["device_launches"]
    s.run_device(d_in, wide.shape[1], F, d_pow)
    d.run_device(d_pow, n_rows, d_rows, d_det)
    assert eng.stats()["device_launches"] == launches + 2                 # one kernel each, nothing between them
    eng.synchronize()
    got = _download(capi, eng, d_rows, d_det, n_rows, K)
    assert np.array_equal(eng.dev_download(d_pow, power.nbytes, np.uint32).reshape(power.shape), power)
    _same(got, want)
    for b in range(n_rows):
        for r, st in zip(got[1][b, :2], dc.STATIONS):
            assert abs(d.offset_hz(dc.RATE, r["centroid_q8"]) - st["offset"]) <= dc.RATE / N
    for p in (d_in, d_pow, d_rows, d_det):
        eng.dev_free(p)
    d.close()
    s.close()
    eng.close()


def test_refusals_queue_nothing(capi, cases, wants):
    c = cases["N64-peaks"]
    want = wants(c.name)
    eng = capi.Engine(1)
    L = capi._lib()
    stats = eng.stats()
    launches, copies = stats["device_launches"], stats["device_copies"]

    def refused(fn, *a, **k):
        with pytest.raises(capi.IqdError) as ei:
            fn(*a, **k)
        assert ei.value.status == -1, (fn, a)
        return str(ei.value)

    # create: every field at both ends of its range, and one past
    good = dict(n_bins=64, floor_rank=63, ratio_q8=256, dc_guard=16, bridge=64, min_width=64, max_detections=32)
    capi.Detector(eng, **good).close()
    capi.Detector(eng, 2048, 0, 2 ** 24, 512, 0, 1, 1024).close()
    capi.Detector(eng, 64, 0, 2 ** 24, 0, 0, 1, 1).close()
    for n in (0, 32, 96, 100, 4096, 2 ** 31):
        assert "n_bins" in refused(capi.Detector, eng, n, 0)
    for field, values in (("floor_rank", (64, 2 ** 32 - 1)), ("ratio_q8", (0, 255, 2 ** 24 + 1, 2 ** 32 - 1)), ("dc_guard", (17, 2 ** 31)),
                          ("bridge", (65, 2 ** 32 - 1)), ("min_width", (0, 65)), ("max_detections", (0, 33, 64))):
        for v in values:
            assert field in refused(capi.Detector, eng, **dict(good, **{field: v})), (field, v)
    h = C.c_void_p()
    cfg = capi.DetectConfig(64, 32, 1024, 0, 0, 1, 4)
    cfg.reserved[0] = 1
    assert L.iqd_detect_create(eng._h, C.byref(cfg), C.byref(h)) == -1 and not h.value
    assert b"reserved" in L.iqd_last_error(eng._h)
    cfg.reserved[0] = 0
    assert L.iqd_detect_create(eng._h, None, C.byref(h)) == -1 and b"cfg" in L.iqd_last_error(eng._h)
    assert L.iqd_detect_create(eng._h, C.byref(cfg), None) == -1 and b"out" in L.iqd_last_error(eng._h)
    assert L.iqd_detect_create(None, C.byref(cfg), C.byref(h)) == -1 and not h.value

    # run
    d = _detector(capi, eng, c.cfg)
    n_rows, K = len(c.power), c.cfg.max_detections
    with pytest.raises(TypeError):
        d.run(c.power.astype(np.int32))
    assert "n_rows" in refused(d.run, np.zeros((0, 64), np.uint32))
    d_in, d_rows, d_det = eng.dev_alloc(c.power.nbytes + 16), eng.dev_alloc(16 * n_rows + 16), eng.dev_alloc(32 * n_rows * K + 16)
    # (the uploads below are the test's own copies; the counters are read after them)
    eng.dev_upload(d_in, c.power.view(np.uint8))
    stats = eng.stats()
    launches, copies = stats["device_launches"], stats["device_copies"]
    for pd, rd, dd, word in ((0, d_rows, d_det, "power"), (d_in, 0, d_det, "rows"), (d_in, d_rows, 0, "det"),
                             (d_in + 4, d_rows, d_det, "power_dev"), (d_in, d_rows + 8, d_det, "rows_dev"),
                             (d_in, d_rows, d_det + 1, "det_dev"), (d_in, d_rows, d_det + 12, "det_dev")):
        assert word in refused(d.run_device, pd, n_rows, rd, dd)
    for n in (0, 2 ** 31, 2 ** 40):
        assert "n_rows" in refused(d.run_device, d_in, n, d_rows, d_det)
    assert L.iqd_detect_run_device(None, C.c_void_p(d_in), n_rows, C.c_void_p(d_rows), C.c_void_p(d_det)) == -1
    assert L.iqd_detect_run(None, C.c_void_p(d_in), n_rows, C.c_void_p(d_rows), C.c_void_p(d_det)) == -1
    rows_h, det_h = np.zeros(n_rows, capi.DETECT_ROW), np.zeros((n_rows, K), capi.DETECTION)
    for args, word in (((None, n_rows, capi._np_ptr(rows_h), capi._np_ptr(det_h)), b"power"),
                       ((capi._np_ptr(c.power), n_rows, None, capi._np_ptr(det_h)), b"rows"),
                       ((capi._np_ptr(c.power), n_rows, capi._np_ptr(rows_h), None), b"det")):
        assert L.iqd_detect_run(d._h, *args) == -1 and word in L.iqd_last_error(eng._h)
    # nothing was queued: no launch and no copy was counted, and the valid calls give the model's numbers
    stats = eng.stats()
    assert (stats["device_launches"], stats["device_copies"]) == (launches, copies)
    d.run_device(d_in, n_rows, d_rows, d_det)
    eng.synchronize()
    _same(_download(capi, eng, d_rows, d_det, n_rows, K), want)
    assert eng.stats()["device_launches"] == launches + 1
    _same(d.run(c.power), want)
    for p in (d_in, d_rows, d_det):
        eng.dev_free(p)
    d.close()
    eng.close()


def _capture(tmp_path, N, F, blocks, rest):
    from rtlsdrdiags_amd import synth
    u8 = synth.wideband(N * F * blocks + rest // 2 + 1, float(dc.RATE), dc.STATIONS, seed=41)[:2 * N * F * blocks + rest]
    cap = tmp_path / "cap.iq"
    u8.tofile(cap)
    return cap, u8[:2 * N * F * blocks].reshape(1, -1)


def test_iqdemod_spectrum_detect_equals_the_python_path(capi, tmp_path):
    """detect= gives one line per detection - block, first / last / centroid offset in Hz, peak dBFS, sum_power - from the
    same numbers as Spectrum.run then Detector.run, on a capture that ends inside a block; out= and log= are what they are
    without detect=; options reach the detector"""
    N, F, blocks, rest = 256, 8, 3, 2 * 256 * 3 + 10
    cap, whole = _capture(tmp_path, N, F, blocks, rest)
    out, log, runs = tmp_path / "power.u32", tmp_path / "spectrum.txt", tmp_path / "runs.txt"
    base = [TOOL, "in=%s" % cap, "rate=%d" % dc.RATE, "bins=%d" % N, "frames=%d" % F, "out=%s" % out, "log=%s" % log]
    eng = capi.Engine(1)
    s = capi.Spectrum(eng, N)
    power = s.run(whole, F)
    p_fs = capi.spectrum_full_scale(N)
    for extra, kw in (([], {}), (["rank=100", "ratio_q8=400", "guard=0", "bridge=2", "minwidth=1", "maxdet=2"],
                                 dict(floor_rank=100, ratio_q8=400, dc_guard=0, bridge=2, min_width=1, max_detections=2))):
        r = subprocess.run(base + ["detect=%s" % runs] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "%d bytes" % rest in r.stderr
        assert out.read_bytes() == power.astype("<u4").tobytes()
        d = capi.Detector(eng, N, **kw)
        rows, det = d.run(power)
        d.close()
        want = []
        for b in range(blocks):
            for rec in det[b, :min(int(rows[b]["n_found"]), d.max_detections)]:
                want.append((b, (int(rec["first_bin"]) - N // 2) * dc.RATE / N, (int(rec["last_bin"]) - N // 2) * dc.RATE / N,
                             capi.detect_offset_hz(N, dc.RATE, rec["centroid_q8"]),
                             float(capi.spectrum_dbfs(rec["peak_power"], p_fs)), int(rec["sum_power"])))
        lines = runs.read_text().splitlines()
        assert len(lines) == len(want) >= 2 * blocks
        for line, w in zip(lines, want):
            blk, lo, hi, hz, db, sp = line.split()
            assert (blk, lo, hi, hz, sp) == ("%d" % w[0], "%.3f" % w[1], "%.3f" % w[2], "%d" % w[3], "%d" % w[5]), (line, w)
            assert abs(float(db) - w[4]) <= 0.006                         # two decimals
        past = int(np.maximum(rows["n_found"].astype(int) - d.max_detections, 0).sum())
        assert ("%d runs past maxdet" % past in r.stderr) == (past > 0)
    assert past > 0                                                       # the second set of options finds more than two
    s.close()
    eng.close()
    bad = subprocess.run(base + ["detect=%s" % runs, "maxdet=1000"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "max_detections" in bad.stderr
    bad = subprocess.run([a.replace("rate=%d" % dc.RATE, "rate=2048000.5") for a in base] + ["detect=%s" % runs],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "whole number" in bad.stderr


def test_iqdemod_spectrum_without_detect_is_unchanged(capi, tmp_path):
    """without detect= the tool writes what it wrote before: out= the API's array, log= one line per block and bin, the
    dropped bytes on stderr and nothing else - and the same bytes as with detect="""
    N, F, blocks, rest = 256, 8, 2, 100
    cap, whole = _capture(tmp_path, N, F, blocks, rest)
    files = {k: (tmp_path / ("power%s.u32" % k), tmp_path / ("spectrum%s.txt" % k)) for k in ("a", "b")}
    runs = tmp_path / "runs.txt"
    res = {}
    for k, extra in (("a", []), ("b", ["detect=%s" % runs])):
        out, log = files[k]
        res[k] = subprocess.run([TOOL, "in=%s" % cap, "rate=%d" % dc.RATE, "bins=%d" % N, "frames=%d" % F, "out=%s" % out,
                                 "log=%s" % log] + extra, capture_output=True, text=True, timeout=120)
        assert res[k].returncode == 0, res[k].stderr
    assert res["a"].stdout == "" and res["a"].stderr == "iqdemod_spectrum: %d bytes after the last whole block dropped\n" % rest
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cap.iq", "powera.u32", "powerb.u32", "runs.txt", "spectruma.txt", "spectrumb.txt"]
    eng = capi.Engine(1)
    s = capi.Spectrum(eng, N)
    want = s.run(whole, F)
    s.close()
    eng.close()
    assert files["a"][0].read_bytes() == want.astype("<u4").tobytes() == files["b"][0].read_bytes()
    text = files["a"][1].read_text()
    assert text == files["b"][1].read_text()
    lines = text.splitlines()
    assert len(lines) == blocks * N
    p_fs = capi.spectrum_full_scale(N)
    for b in range(blocks):
        for k in (0, 1, N // 2, N - 1):
            blk, off, p, db = lines[b * N + k].split()
            assert (int(blk), float(off), int(p)) == (b, (k - N // 2) * dc.RATE / N, int(want[0, b, k]))
            assert abs(float(db) - capi.spectrum_dbfs(want[0, b, k], p_fs)) <= 0.006
