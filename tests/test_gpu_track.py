"""GPU (MI355X): the band activity tracker (include/iqdemod.h: "Band tracks") exactly equal to the Python-int model
(tests/track_model.py) on the inputs of tests/track_cases.py (which tests/test_track_host.py holds to the mutation proof) -
both output arrays in full, in host and device form, split calls, reset, get_state - beside a Detector on one engine,
chained behind Spectrum.run_device and Detector.run_device on one stream, its refusals, and through the iqdemod_spectrum
tool.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import detect_cases as dc
from tests import detect_model as dm
from tests import spectrum_model as sm
from tests import track_cases as tc
from tests import track_model as tm

pytestmark = pytest.mark.gpu
STALE = dm.STALE
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
    return {c.name: c for c in tc.cases(P)}


@pytest.fixture(scope="module")
def wants(cases):
    """name -> the model's two arrays for the case's script of calls, computed once and shared"""
    out = {}

    def get(name):
        if name not in out:
            out[name] = tc.model(cases[name])
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


def _tracker(capi, eng, cfg):
    return capi.Tracker(eng, cfg.n_bins, cfg.n_sources, cfg.max_detections, cfg.n_slots, cfg.gate_q8, cfg.open_hits, cfg.hold_blocks,
                        cfg.alpha_q8, cfg.inc_bias, cfg.class_edge)


class DeviceForm:
    """run(rows, det) through iqd_track_run_device: fresh buffers full of stale bytes for every call, one synchronise"""

    def __init__(self, capi, eng, t, cfg):
        self.capi, self.eng, self.t, self.cfg = capi, eng, t, cfg

    def reset(self):
        self.t.reset()

    def run(self, rows, det):
        cfg, eng = self.cfg, self.eng
        nb = rows.shape[1]
        n_rows = cfg.n_sources * nb
        sizes = (16 * n_rows, 32 * n_rows * cfg.max_detections, 32 * n_rows * cfg.n_slots, 16 * n_rows)
        d_rows, d_det, d_slots, d_blocks = [eng.dev_alloc(n) for n in sizes]
        eng.dev_upload(d_rows, np.ascontiguousarray(rows).view(np.uint8))
        eng.dev_upload(d_det, np.ascontiguousarray(det).view(np.uint8))
        eng.dev_upload(d_slots, np.full(sizes[2], STALE, np.uint8))
        eng.dev_upload(d_blocks, np.full(sizes[3], STALE, np.uint8))
        self.t.run_device(d_rows, d_det, nb, d_slots, d_blocks)
        eng.synchronize()
        slots = eng.dev_download(d_slots, sizes[2]).view(self.capi.TRACK_SLOT).reshape(cfg.n_sources, nb, cfg.n_slots)
        blocks = eng.dev_download(d_blocks, sizes[3]).view(self.capi.TRACK_BLOCK).reshape(cfg.n_sources, nb)
        assert np.array_equal(eng.dev_download(d_det, sizes[1]), np.ascontiguousarray(det).view(np.uint8).ravel())   # only read
        for p in (d_rows, d_det, d_slots, d_blocks):
            eng.dev_free(p)
        return slots, blocks


@pytest.mark.parametrize("name", tc.NAMES)
def test_equal_to_the_model(capi, cases, wants, name):
    """the case's script of calls (split calls and resets among them) in the host form and, on a second tracker, in the
    device form into buffers full of stale bytes; get_state is the last block's slots of every source"""
    c, want = cases[name], wants(name)
    eng = capi.Engine(1)
    th, td = _tracker(capi, eng, c.cfg), _tracker(capi, eng, c.cfg)
    _same(tc.run_script(c, th), want)
    _same(tc.run_script(c, DeviceForm(capi, eng, td, c.cfg)), want)
    for t in (th, td):
        for j in range(c.cfg.n_sources):
            assert t.state(j).tobytes() == want[0][j, -1].tobytes()
    th.close()
    td.close()
    eng.close()


@pytest.mark.parametrize("name", ["N64-S3-life", "N64-sources3", "N2048-K128-S64", "N256-chained"])
def test_a_call_split_in_two_against_the_whole(capi, cases, name):
    """every cut of the case's blocks into two calls gives the model's arrays of one call; after a reset the same again"""
    c = cases[name]
    want = tm.Tracker(c.cfg).run(c.rows, c.det)
    eng = capi.Engine(1)
    t = _tracker(capi, eng, c.cfg)
    for cut in range(1, c.n_blocks, max(1, c.n_blocks // 6)):
        a = t.run(c.rows[:, :cut], c.det[:, :cut])
        b = t.run(c.rows[:, cut:], c.det[:, cut:])
        _same([np.concatenate([a[i], b[i]], axis=1) for i in range(2)], want)
        t.reset()
        assert not t.state(c.cfg.n_sources - 1).view(np.uint8).any()
    _same(t.run(c.rows, c.det), want)
    t.close()
    eng.close()


def test_two_trackers_and_a_detector_on_one_engine(capi, cases, wants):
    """called in turn, block by block; each gives what it gives alone"""
    a, b, dcase = cases["N64-S3-life"], cases["N64-sources3"], {x.name: x for x in dc.cases(capi.channelizer_phasor_table())}["N64-peaks"]
    wa, wb, wd = tm.Tracker(a.cfg).run(a.rows, a.det), tm.Tracker(b.cfg).run(b.rows, b.det), dm.detect(dcase.power, dcase.cfg)
    eng = capi.Engine(1)
    ta, tb = _tracker(capi, eng, a.cfg), _tracker(capi, eng, b.cfg)
    d = capi.Detector(eng, *dcase.cfg)
    got_a, got_b = [], []
    for blk in range(a.n_blocks):
        got_a.append(ta.run(a.rows[:, blk:blk + 1], a.det[:, blk:blk + 1]))
        if blk < b.n_blocks:
            got_b.append(tb.run(b.rows[:, blk:blk + 1], b.det[:, blk:blk + 1]))
        if blk % 6 == 0:
            _same(d.run(dcase.power), wd)
    _same([np.concatenate([g[i] for g in got_a], axis=1) for i in range(2)], wa)
    _same([np.concatenate([g[i] for g in got_b], axis=1) for i in range(2)], wb)
    for o in (ta, tb, d):
        o.close()
    eng.close()


def test_chained_behind_spectrum_and_detector_on_one_stream(capi, P, cases):
    """Spectrum.run_device, Detector.run_device, Tracker.run_device queued back to back, one synchronise at the end, in two
    calls of 10 and 14 blocks: the three models chained.  The tracker reads the detector's arrays where they lie."""
    c = cases["N256-chained"]
    k = tc.CHAINED
    N, F, nb, K, S = k["N"], k["F"], k["blocks"], 16, k["S"]
    wide = tc.chained_wide()
    power = sm.spectrum(wide, "u8", N, F, None, P)
    rows, det = dm.detect(power.reshape(-1, N), dc.readme_cfg(N))
    assert np.array_equal(rows, c.rows[0]) and np.array_equal(det, c.det[0])
    want = tm.Tracker(c.cfg).run(c.rows, c.det)
    eng = capi.Engine(1)
    s, d, t = capi.Spectrum(eng, N), capi.Detector(eng, N), capi.Tracker(eng, N, n_slots=S)     # the defaults are the README line's
    d_in, d_pow = eng.dev_alloc(wide.nbytes), eng.dev_alloc(power.nbytes)
    d_rows, d_det, d_slots, d_blocks = eng.dev_alloc(16 * nb), eng.dev_alloc(32 * nb * K), eng.dev_alloc(32 * nb * S), eng.dev_alloc(16 * nb)
    eng.dev_upload(d_in, wide.view(np.uint8))
    for p, n in ((d_pow, power.nbytes), (d_rows, 16 * nb), (d_det, 32 * nb * K), (d_slots, 32 * nb * S), (d_blocks, 16 * nb)):
        eng.dev_upload(p, np.full(n, STALE, np.uint8))
    launches = eng.stats()["device_launches"]
    block_bytes = 2 * N * F
    for b0, b1 in ((0, 10), (10, 24)):
        n = b1 - b0
        s.run_device(d_in + b0 * block_bytes, n * block_bytes, F, d_pow + b0 * N * 4)
        d.run_device(d_pow + b0 * N * 4, n, d_rows + 16 * b0, d_det + 32 * K * b0)
        t.run_device(d_rows + 16 * b0, d_det + 32 * K * b0, n, d_slots + 32 * S * b0, d_blocks + 16 * b0)
    assert eng.stats()["device_launches"] == launches + 6                 # one kernel each, nothing between them
    eng.synchronize()
    slots = eng.dev_download(d_slots, 32 * nb * S).view(capi.TRACK_SLOT).reshape(1, nb, S)
    blocks = eng.dev_download(d_blocks, 16 * nb).view(capi.TRACK_BLOCK).reshape(1, nb)
    _same((slots, blocks), want)
    # what the host does with a block: the phase_inc column is what set_channels takes
    active = slots[0, 12][slots[0, 12]["state"] == 2]
    assert sorted(capi.detect_offset_hz(N, tc.RATE, int(x["centre_q8"])) // 1000 for x in active) == [-701, 249]
    assert [int(x["phase_inc"]) for x in active] == [capi.track_phase_inc(N, int(x["centre_q8"])) for x in active]
    for p in (d_in, d_pow, d_rows, d_det, d_slots, d_blocks):
        eng.dev_free(p)
    for o in (t, d, s):
        o.close()
    eng.close()


def test_refusals_queue_nothing(capi, cases, wants):
    c = cases["N64-S3-life"]
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
    good = dict(n_bins=64, n_sources=1, max_detections=32, n_slots=64, gate_q8=256 * 64 - 1, open_hits=255, hold_blocks=65535,
                alpha_q8=256, inc_bias=2 ** 32 - 1, class_edge=(1, 1, 65))
    for n in (0, 32, 96, 4096, 2 ** 31):
        assert "n_bins" in refused(capi.Tracker, eng, **dict(good, n_bins=n))
    for field, values in (("n_sources", (0,)), ("max_detections", (0, 33)), ("n_slots", (0, 65, 2 ** 31)), ("gate_q8", (256 * 64, 2 ** 32 - 1)),
                          ("open_hits", (0, 256)), ("hold_blocks", (65536, 2 ** 32 - 1)), ("alpha_q8", (0, 257)),
                          ("class_edge", ((0, 1, 2), (3, 2, 4), (1, 5, 4), (1, 2, 66)))):
        for v in values:
            assert field in refused(capi.Tracker, eng, **dict(good, **{field: v})), (field, v)
    h = C.c_void_p()
    cfg = capi.TrackConfig(1, 64, 4, 3, 512, 3, 2, 64, 0)
    cfg.class_edge[0], cfg.class_edge[1], cfg.class_edge[2] = 2, 4, 16
    for i in range(4):
        cfg.reserved[i] = 1
        assert L.iqd_track_create(eng._h, C.byref(cfg), C.byref(h)) == -1 and not h.value
        assert b"reserved" in L.iqd_last_error(eng._h)
        cfg.reserved[i] = 0
    assert L.iqd_track_create(eng._h, None, C.byref(h)) == -1 and b"cfg" in L.iqd_last_error(eng._h)
    assert L.iqd_track_create(eng._h, C.byref(cfg), None) == -1 and b"out" in L.iqd_last_error(eng._h)
    assert L.iqd_track_create(None, C.byref(cfg), C.byref(h)) == -1 and not h.value
    stats = eng.stats()
    assert (stats["device_launches"], stats["device_copies"]) == (launches, copies)     # a refused create queued nothing
    capi.Tracker(eng, **good).close()
    capi.Tracker(eng, 2048, 3, 1, 1, 0, 1, 0, 1, 0, (2049, 2049, 2049)).close()

    # run
    t, t3 = _tracker(capi, eng, c.cfg), capi.Tracker(eng, 64, n_sources=3)
    nb, K, S = c.n_blocks, c.cfg.max_detections, c.cfg.n_slots
    with pytest.raises(TypeError):
        t.run(c.rows.view(np.uint8), c.det)
    assert "n_blocks" in refused(t.run, c.rows[:, :0], c.det[:, :0])
    ptrs = [eng.dev_alloc(n + 16) for n in (16 * nb, 32 * nb * K, 32 * nb * S, 16 * nb)]
    eng.dev_upload(ptrs[0], c.rows.view(np.uint8))
    eng.dev_upload(ptrs[1], c.det.view(np.uint8))
    stats = eng.stats()
    launches, copies = stats["device_launches"], stats["device_copies"]
    words = ("rows", "det", "slots", "blocks")
    for i, word in enumerate(words):
        for off in (None, 4, 8, 1):
            a = list(ptrs)
            a[i] = 0 if off is None else a[i] + off
            msg = refused(t.run_device, a[0], a[1], nb, a[2], a[3])
            assert word + ("" if off is None else "_dev") in msg, (word, off, msg)
    for n in (0, 2 ** 31, 2 ** 40):
        assert "n_blocks" in refused(t.run_device, ptrs[0], ptrs[1], n, ptrs[2], ptrs[3])
    assert "n_blocks" in refused(t3.run_device, ptrs[0], ptrs[1], (2 ** 31 - 1) // 3 + 1, ptrs[2], ptrs[3])
    assert "source" in refused(t3.state, 3) and "source" in refused(t.state, 1)
    vp = C.c_void_p
    assert L.iqd_track_run_device(None, vp(ptrs[0]), vp(ptrs[1]), nb, vp(ptrs[2]), vp(ptrs[3])) == -1
    assert L.iqd_track_run(None, vp(ptrs[0]), vp(ptrs[1]), nb, vp(ptrs[2]), vp(ptrs[3])) == -1
    assert L.iqd_track_reset(None) == -1 and L.iqd_track_get_state(None, 0, vp(ptrs[2])) == -1
    assert L.iqd_track_get_state(t._h, 0, None) == -1 and b"out" in L.iqd_last_error(eng._h)
    hs, hb = np.zeros((1, nb, S), capi.TRACK_SLOT), np.zeros((1, nb), capi.TRACK_BLOCK)
    host = [capi._np_ptr(c.rows), capi._np_ptr(c.det), capi._np_ptr(hs), capi._np_ptr(hb)]
    for i, word in enumerate(words):
        a = list(host)
        a[i] = None
        assert L.iqd_track_run(t._h, a[0], a[1], nb, a[2], a[3]) == -1 and word.encode() in L.iqd_last_error(eng._h)
    # nothing was queued: no launch and no copy was counted, the state is untouched, and the valid calls give the model's numbers
    stats = eng.stats()
    assert (stats["device_launches"], stats["device_copies"]) == (launches, copies)
    t.run_device(*ptrs[:2], nb, *ptrs[2:])
    eng.synchronize()
    assert eng.stats()["device_launches"] == launches + 1
    got = (eng.dev_download(ptrs[2], 32 * nb * S).view(capi.TRACK_SLOT).reshape(1, nb, S),
           eng.dev_download(ptrs[3], 16 * nb).view(capi.TRACK_BLOCK).reshape(1, nb))
    _same(got, want)
    for p in ptrs:
        eng.dev_free(p)
    t.close()
    t3.close()
    eng.close()


def _tool_capture(tmp_path, rest):
    """the chained case's keyed capture and `rest` bytes more: it ends inside a block"""
    whole = tc.chained_wide()
    cap = tmp_path / "cap.iq"
    np.concatenate([whole[0], np.full(rest, 128, np.uint8)]).tofile(cap)
    return cap, whole


def test_iqdemod_spectrum_track_equals_the_python_path(capi, tmp_path):
    """track= gives one line per slot record that is live or closing - block, slot, id, state, flags, centre offset in Hz,
    phase_inc, first / last offset, class - from the same numbers as Spectrum.run, Detector.run, Tracker.run; options reach
    the tracker; unplaced detections are counted on stderr; track= needs detect="""
    k = tc.CHAINED
    N, F, nb, rest = k["N"], k["F"], k["blocks"], 2 * 256 * 3 + 10
    cap, whole = _tool_capture(tmp_path, rest)
    out, runs, trk = tmp_path / "power.u32", tmp_path / "runs.txt", tmp_path / "tracks.txt"
    base = [TOOL, "in=%s" % cap, "rate=%d" % tc.RATE, "bins=%d" % N, "frames=%d" % F, "out=%s" % out, "detect=%s" % runs]
    eng = capi.Engine(1)
    s, d = capi.Spectrum(eng, N), capi.Detector(eng, N)
    rows, det = d.run(s.run(whole, F))
    for extra, kw in (([], dict(n_slots=8)),
                      (["slots=1", "gate_q8=300", "open=1", "hold=0", "alpha_q8=256", "bias=0x40000000", "edges=2,3,9"],
                       dict(n_slots=1, gate_q8=300, open_hits=1, hold_blocks=0, alpha_q8=256, inc_bias=0x40000000, class_edge=(2, 3, 9)))):
        r = subprocess.run(base + ["track=%s" % trk] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "%d bytes" % rest in r.stderr
        t = capi.Tracker(eng, N, **kw)
        slots, blocks = t.run(rows.reshape(1, nb), det.reshape(1, nb, 16))
        t.close()
        want = []
        for b in range(nb):
            for i, x in enumerate(slots[0, b]):
                if x["track_id"]:
                    want.append("%d %d %d %d %d %d 0x%08x %.3f %.3f %d" % (
                        b, i, x["track_id"], x["state"], x["flags"], capi.detect_offset_hz(N, tc.RATE, int(x["centre_q8"])),
                        x["phase_inc"], (int(x["first_bin"]) - N // 2) * tc.RATE / N, (int(x["last_bin"]) - N // 2) * tc.RATE / N,
                        x["width_class"]))
        assert trk.read_text().splitlines() == want and len(want) >= nb
        past = int(blocks["n_unplaced"].sum())
        assert ("%d detections found no free slot" % past in r.stderr) == (past > 0)
    assert past > 0                                                       # one slot, two stations
    s.close()
    d.close()
    eng.close()
    bad = subprocess.run(base + ["track=%s" % trk, "slots=65"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "n_slots" in bad.stderr
    bad = subprocess.run([a for a in base if not a.startswith("detect=")] + ["track=%s" % trk], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "needs detect=" in bad.stderr


def test_iqdemod_spectrum_without_track_is_unchanged(capi, tmp_path):
    """without track= the tool writes what it writes with it, apart from the tracks file: the same out= and detect= bytes,
    the same stderr, no further file"""
    k = tc.CHAINED
    N, F, rest = k["N"], k["F"], 100
    cap, whole = _tool_capture(tmp_path, rest)
    res, files = {}, {}
    for key, extra in (("a", []), ("b", ["track=%s" % (tmp_path / "tracks.txt")])):
        files[key] = (tmp_path / ("power%s.u32" % key), tmp_path / ("runs%s.txt" % key))
        res[key] = subprocess.run([TOOL, "in=%s" % cap, "rate=%d" % tc.RATE, "bins=%d" % N, "frames=%d" % F, "out=%s" % files[key][0],
                                   "detect=%s" % files[key][1]] + extra, capture_output=True, text=True, timeout=120)
        assert res[key].returncode == 0, res[key].stderr
    assert res["a"].stdout == "" and res["a"].stderr == "iqdemod_spectrum: %d bytes after the last whole block dropped\n" % rest
    assert res["b"].stdout == "" and res["b"].stderr == res["a"].stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cap.iq", "powera.u32", "powerb.u32", "runsa.txt", "runsb.txt", "tracks.txt"]
    assert files["a"][0].read_bytes() == files["b"][0].read_bytes() and files["a"][1].read_bytes() == files["b"][1].read_bytes()
    eng = capi.Engine(1)
    s = capi.Spectrum(eng, N)
    assert files["a"][0].read_bytes() == s.run(whole, F).astype("<u4").tobytes()
    s.close()
    eng.close()
