"""GPU (MI355X): the band track measurements (include/iqdemod.h: "Band track measurements") exactly equal to the direct-sum
model (tests/measure_model.py) on the inputs of tests/measure_cases.py (which tests/test_measure_host.py holds to the mutation
proof) - the whole output array, in host and device form, a second call into the same buffers - chained behind
Spectrum.run_device, Detector.run_device and Tracker.run_device on one stream, its refusals, and through the iqdemod_spectrum
and iqdemod_wide tools.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import detect_cases as dc
from tests import detect_model as dm
from tests import measure_cases as mc
from tests import measure_model as mm
from tests import spectrum_model as sm
from tests import track_model as tm

pytestmark = pytest.mark.gpu
STALE = dm.STALE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECTRUM_TOOL = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_spectrum")
WIDE_TOOL = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_wide")


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in mc.cases()}


@pytest.fixture(scope="module")
def wants(cases):
    """name -> the model's array, computed once and shared"""
    out = {}

    def get(name):
        if name not in out:
            out[name] = mc.model(cases[name])
            out[name].setflags(write=False)
        return out[name]
    return get


def _same(g, w):
    """every record, every byte"""
    assert g.shape == w.shape and g.dtype == w.dtype
    bad = np.argwhere(g != w)
    assert len(bad) == 0, (len(bad), bad[:8], g[tuple(bad[0])], w[tuple(bad[0])])
    assert g.tobytes() == w.tobytes()


def _measure(capi, eng, cfg, **kw):
    return capi.Measure(eng, cfg.n_bins, cfg.n_sources, cfg.n_slots, cfg.dc_guard, cfg.margin, cfg.obw_tail_q16, cfg.carrier_half,
                        cfg.min_sum, cfg.carrier_min_q8, cfg.wide_bins, **kw)


@pytest.mark.parametrize("name", mc.NAMES)
def test_equal_to_the_model(capi, cases, wants, name):
    """the host form; the device form into a buffer full of stale bytes, then a second call into the same buffers; the inputs
    are only read"""
    c, want = cases[name], wants(name)
    eng = capi.Engine(1)
    m = _measure(capi, eng, c.cfg)
    _same(m.run(c.power, c.rows, c.slots), want)
    ins = [np.ascontiguousarray(a).view(np.uint8).ravel() for a in (c.power, c.rows, c.slots)]
    ptrs = [eng.dev_alloc(a.nbytes) for a in ins]
    for p, a in zip(ptrs, ins):
        eng.dev_upload(p, a)
    d_meas = eng.dev_alloc(want.nbytes)
    eng.dev_upload(d_meas, np.full(want.nbytes, STALE, np.uint8))
    for _ in range(2):
        m.run_device(ptrs[0], ptrs[1], ptrs[2], c.n_blocks, d_meas)
        eng.synchronize()
        _same(eng.dev_download(d_meas, want.nbytes).view(capi.TRACK_MEASURE).reshape(want.shape), want)
    for p, a in zip(ptrs, ins):
        assert np.array_equal(eng.dev_download(p, a.nbytes), a)
        eng.dev_free(p)
    eng.dev_free(d_meas)
    m.close()
    eng.close()


def test_chained_behind_spectrum_detector_and_tracker_on_one_stream(capi):
    """Spectrum.run_device, Detector.run_device, Tracker.run_device, Measure.run_device queued back to back, one synchronise at
    the end, in two calls of 2 and 4 blocks: the four models chained.  Under the default thresholds the three stations are
    named CARRIER, NARROW and WIDE."""
    k = mc.THREE
    N, F, nb, S, K = k["N"], k["F"], k["blocks"], k["S"], 16
    wide = mc.three_wide()
    power = sm.spectrum(wide, "u8", N, F, None, capi.channelizer_phasor_table())
    rows, det = dm.detect(power.reshape(-1, N), dc.readme_cfg(N))
    slots, _ = tm.Tracker(tm.Cfg(1, N, K, S, 512, 3, 2, 64, 0, capi.track_default_edges(N))).run(rows.reshape(1, nb), det.reshape(1, nb, K))
    d = capi.measure_defaults(N)
    cfg = mm.Cfg(1, N, S, 1, d["margin"], d["obw_tail_q16"], d["carrier_half"], d["min_sum"], d["carrier_min_q8"], d["wide_bins"])
    want = mm.measure(power.reshape(1, nb, N), rows.reshape(1, nb), slots, cfg)
    eng = capi.Engine(1)
    s, dt, t, m = capi.Spectrum(eng, N), capi.Detector(eng, N), capi.Tracker(eng, N, n_slots=S), capi.Measure(eng, N, n_slots=S)
    sizes = dict(pow=4 * N * nb, rows=16 * nb, det=32 * K * nb, slots=32 * S * nb, blocks=16 * nb, meas=32 * S * nb)
    p = {name: eng.dev_alloc(n) for name, n in sizes.items()}
    for name, n in sizes.items():
        eng.dev_upload(p[name], np.full(n, STALE, np.uint8))
    d_in = eng.dev_alloc(wide.nbytes)
    eng.dev_upload(d_in, wide.view(np.uint8))
    launches = eng.stats()["device_launches"]
    block_bytes = 2 * N * F
    for b0, b1 in ((0, 2), (2, 6)):
        n = b1 - b0
        s.run_device(d_in + b0 * block_bytes, n * block_bytes, F, p["pow"] + 4 * N * b0)
        dt.run_device(p["pow"] + 4 * N * b0, n, p["rows"] + 16 * b0, p["det"] + 32 * K * b0)
        t.run_device(p["rows"] + 16 * b0, p["det"] + 32 * K * b0, n, p["slots"] + 32 * S * b0, p["blocks"] + 16 * b0)
        m.run_device(p["pow"] + 4 * N * b0, p["rows"] + 16 * b0, p["slots"] + 32 * S * b0, n, p["meas"] + 32 * S * b0)
    assert eng.stats()["device_launches"] == launches + 8                 # one kernel each, nothing between them
    eng.synchronize()
    got = eng.dev_download(p["meas"], sizes["meas"]).view(capi.TRACK_MEASURE).reshape(1, nb, S)
    _same(eng.dev_download(p["slots"], sizes["slots"]).view(capi.TRACK_SLOT).reshape(1, nb, S), slots)
    _same(got, want)
    hints = {}
    for x in got[0, nb - 1][got[0, nb - 1]["track_id"] != 0]:
        hz = capi.detect_offset_hz(N, mc.RATE, int(x["centroid_q8"]))
        hints[min(mc.THREE_STATIONS, key=lambda st: abs(st["offset"] - hz))["mode"]] = int(x["hint"])
    assert hints == mc.THREE_HINTS
    for q in list(p.values()) + [d_in]:
        eng.dev_free(q)
    for o in (m, t, dt, s):
        o.close()
    eng.close()


def test_refusals_queue_nothing(capi, cases, wants):
    c = cases["N64-states-overlap"]
    want = wants(c.name)
    eng = capi.Engine(1)
    L = capi._lib()

    def refused(fn, *a, **k):
        with pytest.raises(capi.IqdError) as ei:
            fn(*a, **k)
        assert ei.value.status == -1, (fn, a)
        return str(ei.value)

    # create: every field at both ends of its range, and one past
    stats = eng.stats()
    launches, copies = stats["device_launches"], stats["device_copies"]
    good = dict(n_bins=64, n_sources=1, n_slots=64, dc_guard=16, margin=64, obw_tail_q16=32767, carrier_half=8, min_sum=2 ** 32 - 1,
                carrier_min_q8=256, wide_bins=65)
    for n in (0, 32, 96, 4096, 2 ** 31):
        assert "n_bins" in refused(capi.Measure, eng, **dict(good, n_bins=n))
    for field, values in (("n_sources", (0,)), ("n_slots", (0, 65, 2 ** 31)), ("dc_guard", (17, 2 ** 32 - 1)), ("margin", (65, 2 ** 31)),
                          ("obw_tail_q16", (32768, 65536)), ("carrier_half", (9, 2 ** 31)), ("carrier_min_q8", (257,)),
                          ("wide_bins", (0, 66)), ("reserved", ((1, 0), (0, 1)))):
        for v in values:
            assert field in refused(capi.Measure, eng, **dict(good, **{field: v})), (field, v)
    h = C.c_void_p()
    cfg = capi.MeasureConfig(1, 64, 8, 1, 1, 328, 1, 0, 128, 8)
    assert L.iqd_measure_create(eng._h, None, C.byref(h)) == -1 and b"cfg" in L.iqd_last_error(eng._h)
    assert L.iqd_measure_create(eng._h, C.byref(cfg), None) == -1 and b"out" in L.iqd_last_error(eng._h)
    assert L.iqd_measure_create(None, C.byref(cfg), C.byref(h)) == -1 and not h.value
    stats = eng.stats()
    assert (stats["device_launches"], stats["device_copies"]) == (launches, copies)     # a refused create queued nothing
    capi.Measure(eng, **good).close()
    capi.Measure(eng, 2048, 3, 1, 0, 0, 0, 0, 0, 0, 1).close()

    # run
    m, m3 = _measure(capi, eng, c.cfg), capi.Measure(eng, 64, n_sources=3)
    nb, S = c.n_blocks, c.cfg.n_slots
    with pytest.raises(TypeError):
        m.run(c.power.view(np.int32), c.rows, c.slots)
    assert "n_blocks" in refused(m.run, c.power[:, :0], c.rows[:, :0], c.slots[:, :0])
    ins = [np.ascontiguousarray(a).view(np.uint8).ravel() for a in (c.power, c.rows, c.slots)]
    ptrs = [eng.dev_alloc(a.nbytes + 16) for a in ins] + [eng.dev_alloc(want.nbytes + 16)]
    for p, a in zip(ptrs, ins):
        eng.dev_upload(p, a)
    stats = eng.stats()
    launches, copies = stats["device_launches"], stats["device_copies"]
    words = ("power", "rows", "slots", "meas")

    def dev(a, n=nb, obj=m):
        return obj.run_device(a[0], a[1], a[2], n, a[3])

    for i, word in enumerate(words):
        for off in (None, 4, 8, 1):
            a = list(ptrs)
            a[i] = 0 if off is None else a[i] + off
            msg = refused(dev, a)
            assert word + ("" if off is None else "_dev") in msg, (word, off, msg)
    for n in (0, 2 ** 31, 2 ** 40):
        assert "n_blocks" in refused(dev, ptrs, n)
    assert "n_blocks" in refused(dev, ptrs, (2 ** 31 - 1) // 3 + 1, m3)
    vp = C.c_void_p
    assert L.iqd_measure_run_device(None, vp(ptrs[0]), vp(ptrs[1]), vp(ptrs[2]), nb, vp(ptrs[3])) == -1
    assert L.iqd_measure_run(None, vp(ptrs[0]), vp(ptrs[1]), vp(ptrs[2]), nb, vp(ptrs[3])) == -1
    hm = np.zeros(want.shape, capi.TRACK_MEASURE)
    host = [capi._np_ptr(c.power), capi._np_ptr(c.rows), capi._np_ptr(c.slots), capi._np_ptr(hm)]
    for i, word in enumerate(words):
        a = list(host)
        a[i] = None
        assert L.iqd_measure_run(m._h, a[0], a[1], a[2], nb, a[3]) == -1 and word.encode() in L.iqd_last_error(eng._h)
    # nothing was queued: no launch and no copy was counted, and the valid call gives the model's numbers
    stats = eng.stats()
    assert (stats["device_launches"], stats["device_copies"]) == (launches, copies)
    dev(ptrs)
    eng.synchronize()
    assert eng.stats()["device_launches"] == launches + 1
    _same(eng.dev_download(ptrs[3], want.nbytes).view(capi.TRACK_MEASURE).reshape(want.shape), want)
    for p in ptrs:
        eng.dev_free(p)
    m.close()
    m3.close()
    eng.close()


def _chain(capi, eng, wide, N, F, S, **kw):
    """Spectrum.run, Detector.run, Tracker.run, Measure.run with the tools' defaults: (slots, meas), [blocks, S]"""
    s, d, t, m = capi.Spectrum(eng, N), capi.Detector(eng, N), capi.Tracker(eng, N, n_slots=S), capi.Measure(eng, N, n_slots=S, **kw)
    power = s.run(wide, F)
    nb = power.reshape(-1, N).shape[0]
    rows, det = d.run(power)
    slots, _ = t.run(rows.reshape(1, nb), det.reshape(1, nb, 16))
    meas = m.run(power.reshape(1, nb, N), rows.reshape(1, nb), slots)
    for o in (m, t, d, s):
        o.close()
    return slots[0], meas[0]


def test_iqdemod_spectrum_measure_equals_the_python_path(capi, tmp_path):
    """measure= gives one line per measured record from the same numbers as the Python path, with the defaults and with every
    option set; it needs track=; without it the other files are the same bytes"""
    k = mc.THREE
    N, F, nb, S, rest = k["N"], k["F"], k["blocks"], k["S"], 1000
    cap = tmp_path / "cap.iq"
    wide = mc.three_wide()
    np.concatenate([wide[0], np.full(rest, 128, np.uint8)]).tofile(cap)
    files = {n: tmp_path / n for n in ("power.u32", "runs.txt", "tracks.txt", "meas.txt")}
    base = [SPECTRUM_TOOL, "in=%s" % cap, "rate=%d" % mc.RATE, "bins=%d" % N, "frames=%d" % F, "out=%s" % files["power.u32"],
            "detect=%s" % files["runs.txt"], "track=%s" % files["tracks.txt"]]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    before = {n: files[n].read_bytes() for n in ("power.u32", "runs.txt", "tracks.txt")}
    eng = capi.Engine(1)
    for extra, kw in (([], {}),
                      (["margin=3", "beta_q16=6000", "carrier=0", "minsum=16000000", "carrier_q8=100", "wide=12"],
                       dict(margin=3, obw_tail_q16=6000, carrier_half=0, min_sum=16000000, carrier_min_q8=100, wide_bins=12))):
        r = subprocess.run(base + ["measure=%s" % files["meas.txt"]] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stderr == plain.stderr and r.stdout == ""
        assert {n: files[n].read_bytes() for n in before} == before
        slots, meas = _chain(capi, eng, wide, N, F, S, **kw)
        want = []
        for b in range(nb):
            for i, x in enumerate(meas[b]):
                if x["track_id"]:
                    hz = [capi.detect_offset_hz(N, mc.RATE, 256 * int(x[f]) + 128) for f in ("obw_lo", "obw_hi", "peak_bin")]
                    want.append("%d %d %d %d %d %d %d %d %d %d %d" % (b, i, x["track_id"], hz[0], hz[1], hz[2],
                                capi.detect_offset_hz(N, mc.RATE, int(x["centroid_q8"])), x["carrier_q8"], x["sum_excess"], x["flags"], x["hint"]))
        assert files["meas.txt"].read_text().splitlines() == want and len(want) == 3 * nb
    assert {int(w.split()[-2]) for w in want} == {0, capi.MEASURE_F_WEAK}            # min_sum between the stations' sums
    eng.close()
    bad = subprocess.run(base + ["measure=%s" % files["meas.txt"], "beta_q16=40000"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "obw_tail_q16" in bad.stderr
    bad = subprocess.run([a for a in base if not a.startswith("track=")] + ["measure=%s" % files["meas.txt"]], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "needs track=" in bad.stderr


def test_iqdemod_wide_modes_auto_sets_what_the_python_path_sets(capi, tmp_path):
    """tracks= modes=auto measlog= on the three-station capture, 12 table blocks in calls of 4: the logged records and the
    modes the tool sets are the Python path's - am, fm, wbfm for the three stations, decided in the first call - and every
    station's channel has PCM; without modes=auto and measlog= the tool writes what it wrote"""
    k = mc.THREE
    N, F, S, nb, K = k["N"], k["F"], 3, 12, 4
    wide = mc.three_wide(nb)
    cap = tmp_path / "cap.iq"
    wide[0].tofile(cap)
    base = [WIDE_TOOL, "in=%s" % cap, "rate=%d" % mc.RATE, "tracks=%d" % S, "bins=%d" % N, "frames=%d" % F, "blocks=%d" % K]
    r = subprocess.run(base + ["modes=auto", "out=%s" % (tmp_path / "auto_%d.s16"), "measlog=%s" % (tmp_path / "meas.txt")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    eng = capi.Engine(1)
    slots, meas = _chain(capi, eng, wide, N, F, S)
    eng.close()
    want_m = ["m %d %d %d %d %d %d %d %d" % (b, c, x["track_id"], x["flags"], x["hint"], int(x["obw_hi"]) - int(x["obw_lo"]) + 1,
                                             x["carrier_q8"], x["sum_excess"])
              for b in range(nb) for c, x in enumerate(meas[b]) if x["track_id"]]
    modes = mc.auto_modes(slots, meas, K)
    want_mode = ["mode %d %d %d %d" % t for t in modes]
    lines = (tmp_path / "meas.txt").read_text().splitlines()
    assert [x for x in lines if x.startswith("m ")] == want_m and len(want_m) == 3 * nb
    assert [x for x in lines if x.startswith("mode ")] == want_mode
    by_station = {}
    for b0, c, tid, mode in modes:
        x = meas[b0 + K - 1, c]
        hz = capi.detect_offset_hz(N, mc.RATE, int(x["centroid_q8"]))
        by_station[min(mc.THREE_STATIONS, key=lambda st: abs(st["offset"] - hz))["mode"]] = (b0, capi.MODE[{1: "am", 2: "fm", 3: "wbfm"}[mode]])
    assert by_station == {"am": (0, capi.MODE["am"]), "fm": (0, capi.MODE["fm"]), "wbfm": (0, capi.MODE["wbfm"])}
    sizes = [(tmp_path / ("auto_%d.s16" % c)).stat().st_size for c in range(S)]
    assert min(sizes) > 0, sizes
    # the fixed-mode line is untouched by the new keys: the same PCM with and without measlog=, and no further file
    fixed = {}
    for key, extra in (("a", []), ("b", ["measlog=%s" % (tmp_path / "meas_b.txt")])):
        q = subprocess.run(base + ["modes=2", "out=%s" % (tmp_path / (key + "_%d.s16"))] + extra, capture_output=True, text=True, timeout=120)
        assert q.returncode == 0 and q.stderr == "" and q.stdout == "", q.stderr
        fixed[key] = [(tmp_path / ("%s_%d.s16" % (key, c))).read_bytes() for c in range(S)]
    assert fixed["a"] == fixed["b"] and [x for x in (tmp_path / "meas_b.txt").read_text().splitlines()] == want_m
    # the first call's PCM is the FM start's in every channel (the one-call lag); a station whose mode changed differs later
    auto = [(tmp_path / ("auto_%d.s16" % c)).read_bytes() for c in range(S)]
    changed = [c for c in range(S) if auto[c] != fixed["a"][c]]
    assert sorted(changed) == sorted(c for _, c, _, mode in modes if mode != 2)
    bad = subprocess.run([WIDE_TOOL, "in=%s" % cap, "rate=%d" % mc.RATE, "offsets=0", "modes=auto", "out=%s" % (tmp_path / "x_%d.s16")],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "need tracks=" in bad.stderr
