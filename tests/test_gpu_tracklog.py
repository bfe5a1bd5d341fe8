"""GPU (MI355X): the band track log (include/iqdemod.h: "Band track log") exactly equal to the plain model
(tests/tracklog_model.py) on the scripts of tests/tracklog_cases.py (which tests/test_tracklog_host.py holds to the mutation
proof) - the three output arrays and the state, in host and device form, a second call into the same buffers, split calls,
reset and get_state - chained behind Spectrum, Detector, Tracker and Measure on one stream, its refusals, the iqdemod_spectrum
tool's events= and a seeded slice of 200 random scripts.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import detect_model as dm
from tests import track_cases as tc
from tests import tracklog_cases as lc
from tests import tracklog_model as lm

pytestmark = pytest.mark.gpu
STALE = dm.STALE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECTRUM_TOOL = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_spectrum")


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def cases(capi):
    return {c.name: c for c in lc.cases(capi.channelizer_phasor_table())}


@pytest.fixture(scope="module")
def wants(cases):
    """name -> the model's result, computed once and shared"""
    out = {}

    def get(name):
        if name not in out:
            out[name] = lc.model(cases[name])
        return out[name]
    return get


def _same(g, w):
    """every record, every byte"""
    assert g.shape == w.shape and g.dtype == w.dtype
    if g.tobytes() != w.tobytes():
        bad = np.argwhere(g.reshape(-1).view(np.uint8).reshape(-1, g.dtype.itemsize) != w.reshape(-1).view(np.uint8).reshape(-1, g.dtype.itemsize))
        i = int(bad[0][0])
        raise AssertionError((len(bad), i, g.reshape(-1)[i], w.reshape(-1)[i]))


def _same_result(got, want):
    (g_runs, g_state), (w_runs, w_state) = got, want
    assert len(g_runs) == len(w_runs)
    for g, w in zip(g_runs, w_runs):
        for a, b in zip(g, w):
            _same(a, b)
    for (gs, gg), (ws, wg) in zip(g_state, w_state):
        _same(gs, ws)
        assert gg == wg


def _log(capi, eng, cfg, **kw):
    return capi.TrackLog(eng, cfg.n_sources, cfg.n_slots, cfg.max_events, cfg.min_active, cfg.vote_min, **kw)


class DeviceLog:
    """run(slots, meas) in the device form: the inputs uploaded, the three outputs full of stale bytes beforehand, and a
    second call into the same buffers.  The log is stateful, so the second call is that of a second object which has seen
    the same history; both must leave the same bytes."""

    def __init__(self, capi, eng, cfg):
        self.capi, self.eng, self.cfg = capi, eng, cfg
        self.logs = [_log(capi, eng, cfg), _log(capi, eng, cfg)]

    def reset(self):
        for x in self.logs:
            x.reset()

    def state(self, j):
        a, b = self.logs[0].state(j), self.logs[1].state(j)
        _same(a[0], b[0])
        assert a[1] == b[1]
        return a

    def run(self, slots, meas):
        capi, eng, c = self.capi, self.eng, self.cfg
        nb = slots.shape[1]
        ins = [np.ascontiguousarray(a).view(np.uint8).ravel() for a in (slots, meas)]
        shapes = [((c.n_sources, nb, c.n_slots), capi.TRACK_SUMMARY), ((c.n_sources, c.max_events), capi.TRACK_SUMMARY),
                  ((c.n_sources,), capi.TRACKLOG_COUNTS)]
        sizes = [int(np.prod(s)) * d.itemsize for s, d in shapes]
        ptrs = [eng.dev_alloc(a.nbytes) for a in ins]
        outs = [eng.dev_alloc(n) for n in sizes]
        for p, a in zip(ptrs, ins):
            eng.dev_upload(p, a)
        for p, n in zip(outs, sizes):
            eng.dev_upload(p, np.full(n, STALE, np.uint8))
        got = []
        for x in self.logs:                                               # the second call lands in the first one's buffers
            x.run_device(ptrs[0], ptrs[1], nb, *outs)
            eng.synchronize()
            got.append([eng.dev_download(p, n).view(d).reshape(s) for p, n, (s, d) in zip(outs, sizes, shapes)])
        for a, b in zip(*got):
            _same(a, b)
        for p, a in zip(ptrs, ins):
            assert np.array_equal(eng.dev_download(p, a.nbytes), a)       # the inputs are only read
        for p in ptrs + outs:
            eng.dev_free(p)
        return tuple(got[0])

    def close(self):
        for x in self.logs:
            x.close()


@pytest.mark.parametrize("name", lc.NAMES)
def test_equal_to_the_model(capi, cases, wants, name):
    """the case's script of calls and resets in the host form and in the device form (stale output buffers, a second call
    into them): summaries, events, counts and the final state, byte for byte"""
    c, want = cases[name], wants(name)
    eng = capi.Engine(1)
    host = _log(capi, eng, c.cfg)
    _same_result(lc.run_script(c, host), want)
    host.close()
    dev = DeviceLog(capi, eng, c.cfg)
    _same_result(lc.run_script(c, dev), want)
    dev.close()
    eng.close()


def test_split_calls_reset_and_get_state(capi, cases):
    """one call of all the blocks against calls of one block each (E large enough): the same summaries and state, the events
    concatenated, the counts summed; get_state between the calls is the model's; reset gives a fresh object's bytes"""
    c = cases["S8-calls"]
    cfg = c.cfg._replace(max_events=256)
    eng = capi.Engine(1)
    whole, parts, model = _log(capi, eng, cfg), _log(capi, eng, cfg), lm.TrackLog(cfg)
    summary, events, counts = whole.run(c.slots, c.meas)
    got = []
    for b in range(c.n_blocks):
        got.append(parts.run(c.slots[:, b:b + 1], c.meas[:, b:b + 1]))
        model.run(c.slots[:, b:b + 1], c.meas[:, b:b + 1])
        st, g = parts.state(0)
        _same(st, model.state(0)[0])
        assert g == b + 1
    _same(np.concatenate([p[0] for p in got], axis=1), summary)
    _same(np.concatenate([p[1][0, :p[2][0]["n_stored"]] for p in got]), events[0, :counts[0]["n_stored"]])
    for f in capi.TRACKLOG_COUNTS.names:
        assert sum(int(p[2][0][f]) for p in got) == counts[0][f]
    _same(parts.state(0)[0], whole.state(0)[0])
    assert whole.state(0)[0]["track_id"].any()
    whole.reset()
    st, g = whole.state(0)
    assert g == 0 and not st.view(np.uint8).any()
    again = whole.run(c.slots, c.meas)
    for a, b in zip(again, (summary, events, counts)):
        _same(a, b)
    for o in (whole, parts):
        o.close()
    eng.close()


def test_chained_behind_the_four_on_one_stream(capi, cases, wants):
    """Spectrum, Detector, Tracker, Measure and TrackLog run_device queued back to back, one synchronise at the end, in the
    chained case's calls of 10, 10 and 4 blocks: the five models chained - the keyed station's one event in the second call"""
    k = tc.CHAINED
    N, F, nb, S, K, E = k["N"], k["F"], k["blocks"], k["S"], 16, 256
    c, (w_runs, w_state) = cases["N256-chained"], wants("N256-chained")
    wide = tc.chained_wide()
    eng = capi.Engine(1)
    s, dt = capi.Spectrum(eng, N), capi.Detector(eng, N)
    t = capi.Tracker(eng, N, n_slots=S, gate_q8=k["G"], open_hits=k["H"], hold_blocks=k["B"], alpha_q8=k["A"],
                     class_edge=tc.chained_cfg().class_edge)
    m, lg = capi.Measure(eng, N, n_slots=S), capi.TrackLog(eng, n_slots=S, max_events=E)
    calls = [(op[1], op[2]) for op in c.calls]
    sizes = dict(pow=4 * N * nb, rows=16 * nb, det=32 * K * nb, slots=32 * S * nb, blocks=16 * nb, meas=32 * S * nb, summary=64 * S * nb,
                 events=64 * E * len(calls), counts=16 * len(calls))
    p = {name: eng.dev_alloc(n) for name, n in sizes.items()}
    for name, n in sizes.items():
        eng.dev_upload(p[name], np.full(n, STALE, np.uint8))
    d_in = eng.dev_alloc(wide.nbytes)
    eng.dev_upload(d_in, wide.view(np.uint8))
    launches = eng.stats()["device_launches"]
    block_bytes = 2 * N * F
    for i, (b0, b1) in enumerate(calls):
        n = b1 - b0
        s.run_device(d_in + b0 * block_bytes, n * block_bytes, F, p["pow"] + 4 * N * b0)
        dt.run_device(p["pow"] + 4 * N * b0, n, p["rows"] + 16 * b0, p["det"] + 32 * K * b0)
        t.run_device(p["rows"] + 16 * b0, p["det"] + 32 * K * b0, n, p["slots"] + 32 * S * b0, p["blocks"] + 16 * b0)
        m.run_device(p["pow"] + 4 * N * b0, p["rows"] + 16 * b0, p["slots"] + 32 * S * b0, n, p["meas"] + 32 * S * b0)
        lg.run_device(p["slots"] + 32 * S * b0, p["meas"] + 32 * S * b0, n, p["summary"] + 64 * S * b0, p["events"] + 64 * E * i,
                      p["counts"] + 16 * i)
    assert eng.stats()["device_launches"] == launches + 5 * len(calls)     # one kernel each, nothing between them
    eng.synchronize()
    _same(eng.dev_download(p["slots"], sizes["slots"]).view(capi.TRACK_SLOT).reshape(1, nb, S), c.slots)
    _same(eng.dev_download(p["meas"], sizes["meas"]).view(capi.TRACK_MEASURE).reshape(1, nb, S), c.meas)
    _same(eng.dev_download(p["summary"], sizes["summary"]).view(capi.TRACK_SUMMARY).reshape(1, nb, S),
          np.concatenate([r[0] for r in w_runs], axis=1))
    events = eng.dev_download(p["events"], sizes["events"]).view(capi.TRACK_SUMMARY).reshape(len(calls), 1, E)
    counts = eng.dev_download(p["counts"], sizes["counts"]).view(capi.TRACKLOG_COUNTS).reshape(len(calls), 1)
    for i, r in enumerate(w_runs):
        _same(events[i], r[1])
        _same(counts[i], r[2])
    assert [int(x["n_events"]) for x in counts[:, 0]] == [0, 1, 0] and events[1, 0, 0]["track_id"] == 2
    st, g = lg.state(0)
    _same(st, w_state[0][0])
    assert g == nb
    for q in list(p.values()) + [d_in]:
        eng.dev_free(q)
    for o in (lg, m, t, dt, s):
        o.close()
    eng.close()


def test_refusals_queue_nothing(capi, cases, wants):
    c = cases["S1-life"]
    (want,), _ = wants(c.name)
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
    good = dict(n_sources=1, n_slots=64, max_events=65536, min_active=65535, vote_min=65535)
    for field, values in (("n_sources", (0,)), ("n_slots", (0, 65, 2 ** 31)), ("max_events", (0, 65537, 2 ** 32 - 1)),
                          ("min_active", (0, 65536, 2 ** 31)), ("vote_min", (0, 65536, 2 ** 32 - 1)),
                          ("reserved", ((1, 0, 0), (0, 1, 0), (0, 0, 1)))):
        for v in values:
            assert field in refused(capi.TrackLog, eng, **dict(good, **{field: v})), (field, v)
    h = C.c_void_p()
    cfg = capi.TrackLogConfig(1, 8, 16, 2, 4)
    assert L.iqd_tracklog_create(eng._h, None, C.byref(h)) == -1 and b"cfg" in L.iqd_last_error(eng._h)
    assert L.iqd_tracklog_create(eng._h, C.byref(cfg), None) == -1 and b"out" in L.iqd_last_error(eng._h)
    assert L.iqd_tracklog_create(None, C.byref(cfg), C.byref(h)) == -1 and not h.value
    stats = eng.stats()
    assert (stats["device_launches"], stats["device_copies"]) == (launches, copies)     # a refused create queued nothing
    capi.TrackLog(eng, **good).close()
    capi.TrackLog(eng, 3, 1, 1, 1, 1).close()

    # run and get_state
    lg, lg3 = _log(capi, eng, c.cfg), capi.TrackLog(eng, 3, 1)
    nb = c.n_blocks
    with pytest.raises(TypeError):
        lg.run(c.slots.view(np.uint8), c.meas)
    assert "n_blocks" in refused(lg.run, c.slots[:, :0], c.meas[:, :0])
    ins = [np.ascontiguousarray(a).view(np.uint8).ravel() for a in (c.slots, c.meas)]
    sizes = [a.nbytes for a in ins] + [x.nbytes for x in want]
    ptrs = [eng.dev_alloc(n + 16) for n in sizes]
    for p, a in zip(ptrs, ins):
        eng.dev_upload(p, a)
    stats = eng.stats()
    launches, copies = stats["device_launches"], stats["device_copies"]
    words = ("slots", "meas", "summary", "events", "counts")

    def dev(a, n=nb, obj=lg):
        return obj.run_device(a[0], a[1], n, a[2], a[3], a[4])

    for i, word in enumerate(words):
        for off in (None, 4, 8, 1):
            a = list(ptrs)
            a[i] = 0 if off is None else a[i] + off
            msg = refused(dev, a)
            assert word + ("" if off is None else "_dev") in msg, (word, off, msg)
    for n in (0, 2 ** 31, 2 ** 40):
        assert "n_blocks" in refused(dev, ptrs, n)
    assert "n_blocks" in refused(dev, ptrs, (2 ** 31 - 1) // 3 + 1, lg3)
    assert "source" in refused(lg.state, 1) and "source" in refused(lg3.state, 3)
    vp = C.c_void_p
    args = [vp(ptrs[0]), vp(ptrs[1]), nb, vp(ptrs[2]), vp(ptrs[3]), vp(ptrs[4])]
    assert L.iqd_tracklog_run_device(None, *args) == -1 and L.iqd_tracklog_run(None, *args) == -1 and L.iqd_tracklog_reset(None) == -1
    g = C.c_uint64()
    one = np.zeros(1, capi.TRACK_SUMMARY)
    assert L.iqd_tracklog_get_state(None, 0, capi._np_ptr(one), C.byref(g)) == -1
    assert L.iqd_tracklog_get_state(lg._h, 0, None, C.byref(g)) == -1 and b"out" in L.iqd_last_error(eng._h)
    assert L.iqd_tracklog_get_state(lg._h, 0, capi._np_ptr(one), None) == -1 and b"next_block" in L.iqd_last_error(eng._h)
    hs = [np.zeros(x.shape, x.dtype) for x in want]
    host = [capi._np_ptr(c.slots), capi._np_ptr(c.meas)] + [capi._np_ptr(x) for x in hs]
    for i, word in enumerate(words):
        a = list(host)
        a[i] = None
        assert L.iqd_tracklog_run(lg._h, a[0], a[1], nb, a[2], a[3], a[4]) == -1 and word.encode() in L.iqd_last_error(eng._h)
    # nothing was queued: no launch and no copy was counted, the state is untouched, and the valid call gives the model's bytes
    stats = eng.stats()
    assert (stats["device_launches"], stats["device_copies"]) == (launches, copies)
    dev(ptrs)
    eng.synchronize()
    assert eng.stats()["device_launches"] == launches + 1
    for p, x in zip(ptrs[2:], want):
        _same(eng.dev_download(p, x.nbytes).view(x.dtype).reshape(x.shape), x)
    for p in ptrs:
        eng.dev_free(p)
    lg.close()
    lg3.close()
    eng.close()


def _event_lines(capi, N, F, rate, summary_runs, state):
    """what iqdemod_spectrum events= writes, from the Python path's numbers: the events of every call with their slots (found
    in the summaries: the closing record, or the block in which the id left its slot), then the open tracks"""
    sec = N * F / rate

    def line(slot, r, word):
        n_act, n_meas = int(r["n_active"]), int(r["n_measured"])
        cen = capi.detect_offset_hz(N, rate, capi.tracklog_mean_centre(int(r["sum_centre_q8"]), n_act)) if n_act else 0
        lo = capi.detect_offset_hz(N, rate, 256 * int(r["obw_lo_min"]) + 128) if n_meas else 0
        hi = capi.detect_offset_hz(N, rate, 256 * int(r["obw_hi_max"]) + 128) if n_meas else 0
        return "%d %d %d %d %.6f %.6f %d %d %d %d %d %d %d %d %d %d%s" % (
            r["track_id"], slot, r["first_block"], r["n_blocks"], int(r["first_block"]) * sec, int(r["n_blocks"]) * sec, cen, lo, hi,
            r["mode_hint"], r["votes"][0], r["votes"][1], r["votes"][2], n_meas, int(r["sum_excess"]) // n_meas if n_meas else 0, r["flags"], word)

    out = []
    for summary, events, counts in summary_runs:
        for e in events[0, :counts[0]["n_stored"]]:
            if e["flags"] & lm.F_CLOSED:
                at = np.argwhere((summary[0]["track_id"] == e["track_id"]) & ((summary[0]["flags"] & lm.F_CLOSED) != 0))
            else:
                raise AssertionError("the tracker's own tables lose no track")
            assert len(at) == 1
            out.append(line(int(at[0][1]), e, ""))
    live, _ = state
    out += [line(i, r, " open") for i, r in enumerate(live) if r["track_id"]]
    return out


def _python_chain(capi, eng, wide, N, F, S, **kw):
    """Spectrum.run, Detector.run, Tracker.run, Measure.run, TrackLog.run in one call with the tools' defaults"""
    s, d, t, m = capi.Spectrum(eng, N), capi.Detector(eng, N), capi.Tracker(eng, N, n_slots=S), capi.Measure(eng, N, n_slots=S)
    lg = capi.TrackLog(eng, n_slots=S, **kw)
    power = s.run(wide, F)
    nb = power.reshape(-1, N).shape[0]
    rows, det = d.run(power)
    slots, _ = t.run(rows.reshape(1, nb), det.reshape(1, nb, 16))
    meas = m.run(power.reshape(1, nb, N), rows.reshape(1, nb), slots)
    run = lg.run(slots, meas)
    state = lg.state(0)
    for o in (lg, m, t, d, s):
        o.close()
    return run, state


def test_iqdemod_spectrum_events_equals_the_python_path(capi, tmp_path):
    """events= writes the chained capture's one event - the keyed station: slot 1, id 2, blocks 6 .. 16, near +250 kHz,
    carrier - and the station still on as `open`; with other settings the Python path's lines again; a capture cut while the
    keyed station is on ends with two tracks open; the other files are the same bytes with and without events=; it needs
    track= and measure="""
    k = tc.CHAINED
    N, F, S = k["N"], k["F"], k["S"]
    wide = tc.chained_wide()
    eng = capi.Engine(1)
    for blocks, extra, kw, n_events, n_open in ((24, [], {}, 1, 1), (24, ["minactive=10", "votemin=12", "maxevents=1"],
                                                                   dict(min_active=10, vote_min=12, max_events=1), 0, 1),
                                                (12, ["votemin=1"], dict(vote_min=1), 0, 2)):
        cap = tmp_path / ("cap%d.iq" % blocks)
        wide[0, :2 * N * F * blocks].tofile(cap)
        files = {n: tmp_path / n for n in ("power.u32", "runs.txt", "tracks.txt", "meas.txt", "events.txt")}
        base = [SPECTRUM_TOOL, "in=%s" % cap, "rate=%d" % tc.RATE, "bins=%d" % N, "frames=%d" % F, "out=%s" % files["power.u32"],
                "detect=%s" % files["runs.txt"], "track=%s" % files["tracks.txt"], "slots=%d" % S, "measure=%s" % files["meas.txt"]]
        plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
        assert plain.returncode == 0, plain.stderr
        before = {n: files[n].read_bytes() for n in ("power.u32", "runs.txt", "tracks.txt", "meas.txt")}
        r = subprocess.run(base + ["events=%s" % files["events.txt"]] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stderr == plain.stderr and r.stdout == ""
        assert {n: files[n].read_bytes() for n in before} == before
        run, state = _python_chain(capi, eng, wide[:, :2 * N * F * blocks], N, F, S, **kw)
        want = _event_lines(capi, N, F, tc.RATE, [run], state)
        got = files["events.txt"].read_text().splitlines()
        assert got == want
        assert (len([x for x in got if not x.endswith(" open")]), len([x for x in got if x.endswith(" open")])) == (n_events, n_open)
        if not extra:
            f = got[0].split()
            assert f[:4] == ["2", "1", "6", "11"] and abs(int(f[6]) - 250000) <= tc.RATE // N and f[9] == "1" and f[15] == str(lm.F_CLOSED)
            assert (float(f[4]), float(f[5])) == (round(6 * N * F / tc.RATE, 6), round(11 * N * F / tc.RATE, 6))
            o = got[1].split()
            assert o[:4] == ["1", "0", "0", "24"] and abs(int(o[6]) + 700000) <= tc.RATE // N and o[-1] == "open"
    eng.close()
    bad = subprocess.run(base + ["events=%s" % files["events.txt"], "votemin=0"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "vote_min" in bad.stderr
    for drop in ("measure=", "track="):
        args = [a for a in base if not a.startswith(drop) and not (drop == "track=" and a.startswith("measure="))]
        bad = subprocess.run(args + ["events=%s" % files["events.txt"]], capture_output=True, text=True, timeout=120)
        assert bad.returncode == 1 and "needs track= and measure=" in bad.stderr


@pytest.fixture(scope="module")
def fuzz():
    cs = lc.fuzz_cases()
    return cs, [lc.model(c) for c in cs]


@pytest.mark.parametrize("part", range(4))
def test_seeded_random_scripts(capi, fuzz, part):
    """the fixed-seed slice of 200 random scripts (tests/test_tracklog_host.py counts what it holds), 50 per part, none
    skipped: every script in the host form and in the device form"""
    cs, want = fuzz
    eng = capi.Engine(1)
    ran = 0
    for i in range(part * 50, part * 50 + 50):
        c = cs[i]
        lg = _log(capi, eng, c.cfg)
        _same_result(lc.run_script(c, lg), want[i])
        lg.close()
        dev = DeviceLog(capi, eng, c.cfg)
        _same_result(lc.run_script(c, dev), want[i])
        dev.close()
        ran += 1
    assert ran == 50
    eng.close()
