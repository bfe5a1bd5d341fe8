"""Every refusal of the five band objects (Spectrum, Detector, Tracker, Measure, TrackLog) as a table {label: [status, text]},
made on one engine through the raw library and through rtlsdrdiags_amd.capi at N = 64, S = 8, one block: create (NULLs, every
config field one past each end of its range, every reserved entry), run and run_device (object NULL, each argument NULL, each
device pointer misaligned by 4, the count at 0, 2^31 and 2^40, three sources overflowing, the spectrum's frames_per_block and
bytes_per_source), get_state, and double faults that pin which refusal wins.  A raw call records iqd_last_error's text, a capi
call the IqdError's; a call with a NULL object or engine must leave the engine's last error as it was and records that.
Nothing is launched until the table is complete; then one valid run_device per object, chained, counts its launches.

tests/golden/band_refusals.json is this table as the library gave it before its host code was folded onto
csrc/iqd_band_host.h:  python -m tests.band_refusals tests/golden/band_refusals.json  (on the GPU)."""
import ctypes as C
import json
import sys

import numpy as np

N, S, D, E, F, NB, SRC = 64, 8, 4, 4, 2, 1, 2          # bins, slots, detections per row, events per source, frames, blocks, sources
UNTOUCHED = "(last error untouched)"
N_BINS = (0, 32, 96, 100, 4096, 2 ** 31)

# the pool of arrays the calls share, in bytes; a device array has 16 more, so that a pointer moved by 4 stays inside
SIZES = dict(wide=SRC * NB * 2 * N * F, power=SRC * NB * N * 4, rows=SRC * NB * 16, det=SRC * NB * D * 32, slots=SRC * NB * S * 32,
             blocks=SRC * NB * 16, meas=SRC * NB * S * 32, summary=SRC * NB * S * 64, events=SRC * E * 64, counts=SRC * 16)

# per object: the C names, the run's pointer arguments in the ABI's order, how they and the count make the argument list, the
# counts a run refuses (the first one is the double faults' "count is 0") and the one a valid call takes
RUNS = {
    "spectrum": dict(args=("wide", "power"), order=lambda p, n: (p["wide"], n[0], n[1], p["power"]), valid=(NB * 2 * N * F, F),
                     counts={"frames=0": (NB * 2 * N * F, 0), "frames=2^24+1": (NB * 2 * N * F, 2 ** 24 + 1), "frames=2^32-1": (NB * 2 * N * F, 2 ** 32 - 1),
                             "bytes=0": (0, F), "bytes=a frame short": (NB * 2 * N * F - 2 * N, F), "bytes=2^38": (2 ** 38, 1)}),
    "detect": dict(args=("power", "rows", "det"), order=lambda p, n: (p["power"], n, p["rows"], p["det"]), valid=SRC * NB,
                   counts={"n=0": 0, "n=2^31": 2 ** 31, "n=2^40": 2 ** 40}),
    "track": dict(args=("rows", "det", "slots", "blocks"), order=lambda p, n: (p["rows"], p["det"], n, p["slots"], p["blocks"]), valid=NB,
                  counts={"n=0": 0, "n=2^31": 2 ** 31, "n=2^40": 2 ** 40}),
    "measure": dict(args=("power", "rows", "slots", "meas"), order=lambda p, n: (p["power"], p["rows"], p["slots"], n, p["meas"]), valid=NB,
                    counts={"n=0": 0, "n=2^31": 2 ** 31, "n=2^40": 2 ** 40}),
    "tracklog": dict(args=("slots", "meas", "summary", "events", "counts"), valid=NB,
                     order=lambda p, n: (p["slots"], p["meas"], n, p["summary"], p["events"], p["counts"]),
                     counts={"n=0": 0, "n=2^31": 2 ** 31, "n=2^40": 2 ** 40}),
}

# create: a config every field of which is at an end of its range, and the values one past each end (those of the refusal tests
# in tests/test_gpu_{spectrum,detect,track,measure,tracklog}.py)
CREATES = {
    "spectrum": dict(good=dict(n_sources=1, n_bins=N, sample_format=0), n_reserved=3,
                     fields=(("n_sources", (0,)), ("n_bins", N_BINS), ("sample_format", (2, 3, 2 ** 32 - 1)))),
    "detect": dict(good=dict(n_bins=N, floor_rank=63, ratio_q8=256, dc_guard=16, bridge=64, min_width=64, max_detections=32), n_reserved=1,
                   fields=(("n_bins", N_BINS), ("floor_rank", (64, 2 ** 32 - 1)), ("ratio_q8", (0, 255, 2 ** 24 + 1, 2 ** 32 - 1)),
                           ("dc_guard", (17, 2 ** 31)), ("bridge", (65, 2 ** 32 - 1)), ("min_width", (0, 65)), ("max_detections", (0, 33, 64)))),
    "track": dict(good=dict(n_sources=1, n_bins=N, max_detections=32, n_slots=64, gate_q8=256 * N - 1, open_hits=255, hold_blocks=65535,
                            alpha_q8=256, inc_bias=2 ** 32 - 1, class_edge=(1, 1, 65)), n_reserved=4,
                  fields=(("n_bins", N_BINS), ("n_sources", (0,)), ("max_detections", (0, 33)), ("n_slots", (0, 65, 2 ** 31)),
                          ("gate_q8", (256 * N, 2 ** 32 - 1)), ("open_hits", (0, 256)), ("hold_blocks", (65536, 2 ** 32 - 1)),
                          ("alpha_q8", (0, 257)), ("class_edge", ((0, 1, 2), (3, 2, 4), (1, 5, 4), (1, 2, 66))))),
    "measure": dict(good=dict(n_sources=1, n_bins=N, n_slots=64, dc_guard=16, margin=64, obw_tail_q16=32767, carrier_half=8,
                              min_sum=2 ** 32 - 1, carrier_min_q8=256, wide_bins=65), n_reserved=2,
                    fields=(("n_bins", N_BINS), ("n_sources", (0,)), ("n_slots", (0, 65, 2 ** 31)), ("dc_guard", (17, 2 ** 32 - 1)),
                            ("margin", (65, 2 ** 31)), ("obw_tail_q16", (32768, 65536)), ("carrier_half", (9, 2 ** 31)),
                            ("carrier_min_q8", (257,)), ("wide_bins", (0, 66)))),
    "tracklog": dict(good=dict(n_sources=1, n_slots=64, max_events=65536, min_active=65535, vote_min=65535), n_reserved=3,
                     fields=(("n_sources", (0,)), ("n_slots", (0, 65, 2 ** 31)), ("max_events", (0, 65537, 2 ** 32 - 1)),
                             ("min_active", (0, 65536, 2 ** 31)), ("vote_min", (0, 65536, 2 ** 32 - 1)))),
}


def _config(capi, name, values, reserved=None):
    cfg = {"spectrum": capi.SpectrumConfig, "detect": capi.DetectConfig, "track": capi.TrackConfig, "measure": capi.MeasureConfig,
           "tracklog": capi.TrackLogConfig}[name]()
    for k, v in values.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(cfg, k)[i] = x
        else:
            setattr(cfg, k, v)
    if reserved is not None:
        cfg.reserved[reserved] = 1
    return cfg


def _class(capi, name):
    return {"spectrum": capi.Spectrum, "detect": capi.Detector, "track": capi.Tracker, "measure": capi.Measure, "tracklog": capi.TrackLog}[name]


def _objects(capi, eng, n_sources):
    """the five, as the chain sets them up; the detector has no sources"""
    return {"spectrum": capi.Spectrum(eng, N, n_sources), "detect": capi.Detector(eng, N, max_detections=D),
            "track": capi.Tracker(eng, N, n_sources, max_detections=D, n_slots=S), "measure": capi.Measure(eng, N, n_sources, n_slots=S),
            "tracklog": capi.TrackLog(eng, n_sources, S, max_events=E)}


def collect(capi):
    """-> dict(table={label: [status, text]}, moved=(device_launches, device_copies) counted while the table was made,
    valid={object: device_launches one valid run_device counted})"""
    L = capi._lib()
    eng = capi.Engine(1)
    table = {}

    def put(label, entry):
        assert label not in table, label
        table[label] = entry

    def raw(label, fn, *args, untouched=False):
        before = L.iqd_last_error(eng._h)
        rc = fn(*args)
        text = L.iqd_last_error(eng._h).decode()
        put(label, [rc, UNTOUCHED if untouched and text == before.decode() else text])

    def wrapped(label, fn, *args, **kw):
        try:
            made = fn(*args, **kw)
        except capi.IqdError as err:
            put(label, [err.status, str(err)])
        else:
            put(label, [0, ""])
            if hasattr(made, "close"):
                made.close()

    objs, objs3 = _objects(capi, eng, SRC), _objects(capi, eng, 3)
    rng = np.random.default_rng(64)
    host = {k: np.zeros(n, np.uint8) for k, n in SIZES.items()}
    host["wide"][:] = rng.integers(118, 138, SIZES["wide"])
    dev = {k: eng.dev_alloc(n + 16) for k, n in SIZES.items()}
    for k in dev:
        eng.dev_upload(dev[k], np.zeros(SIZES[k] + 16, np.uint8))
    eng.dev_upload(dev["wide"], host["wide"])
    eng.synchronize()
    stats = eng.stats()
    start = (stats["device_launches"], stats["device_copies"])

    # ---- create -----------------------------------------------------------------------------------------------------------
    for name, c in CREATES.items():
        create = getattr(L, "iqd_%s_create" % name)
        h = C.c_void_p()
        good = _config(capi, name, c["good"])
        raw("%s.create.raw.cfg NULL" % name, create, eng._h, None, C.byref(h))
        raw("%s.create.raw.out NULL" % name, create, eng._h, C.byref(good), None)
        raw("%s.create.raw.out and cfg NULL" % name, create, eng._h, None, None)
        raw("%s.create.raw.engine NULL" % name, create, None, C.byref(good), C.byref(h), untouched=True)
        for field, values in c["fields"]:
            for v in values:
                cfg = _config(capi, name, dict(c["good"], **{field: v}))
                raw("%s.create.raw.%s=%r" % (name, field, v), create, eng._h, C.byref(cfg), C.byref(h))
                if name != "spectrum":
                    wrapped("%s.create.capi.%s=%r" % (name, field, v), _class(capi, name), eng, **dict(c["good"], **{field: v}))
        for i in range(c["n_reserved"]):
            cfg = _config(capi, name, c["good"], reserved=i)
            raw("%s.create.raw.reserved[%d]" % (name, i), create, eng._h, C.byref(cfg), C.byref(h))
            if name in ("measure", "tracklog"):
                r = tuple(int(j == i) for j in range(c["n_reserved"]))
                wrapped("%s.create.capi.reserved[%d]" % (name, i), _class(capi, name), eng, **dict(c["good"], reserved=r))
        put("%s.create.raw.handle" % name, [0, "still NULL" if not h.value else "set"])
    # a bad field together with a reserved entry: the field's text wins
    cfg = _config(capi, "track", dict(CREATES["track"]["good"], alpha_q8=0), reserved=0)
    raw("track.create.raw.alpha_q8=0 and reserved[0]", L.iqd_track_create, eng._h, C.byref(cfg), C.byref(C.c_void_p()))
    # the spectrum through capi, and its window
    wrapped("spectrum.create.capi.n_sources=0", capi.Spectrum, eng, N, n_sources=0)
    for n in N_BINS:
        wrapped("spectrum.create.capi.n_bins=%d" % n, capi.Spectrum, eng, n)
    wrapped("spectrum.create.capi.sample_format=s16", capi.Spectrum, eng, N, sample_format="s16")
    w = np.zeros(N, np.int16)
    for bad in (32640, -32640):
        w[5] = bad
        wrapped("spectrum.create.capi.window[5]=%d" % bad, capi.Spectrum, eng, N, window=w)
    wrapped("spectrum.create.capi.window sum", capi.Spectrum, eng, 1024, window=np.full(1024, 8192, np.int16))

    # ---- run and run_device -------------------------------------------------------------------------------------------------
    for name, r in RUNS.items():
        o, o3 = objs[name], objs3[name]
        run, run_device = getattr(L, "iqd_%s_run" % name), getattr(L, "iqd_%s_run_device" % name)
        hp = {k: host[k].ctypes.data for k in r["args"]}
        dp = {k: dev[k] for k in r["args"]}
        first, second = r["args"][:2]
        zero_label, zero = next(iter(r["counts"].items()))
        forms = (("run.raw", lambda p, n: run(o._h, *r["order"](p, n)), hp), ("run_device.raw", lambda p, n: run_device(o._h, *r["order"](p, n)), dp))
        for form, call, p in forms:
            raw("%s.%s.object NULL" % (name, form), {"run.raw": run, "run_device.raw": run_device}[form], None, *r["order"](p, r["valid"]),
                untouched=True)
            for k in r["args"]:
                raw("%s.%s.%s NULL" % (name, form, k), call, dict(p, **{k: None}), r["valid"])
            for label, n in r["counts"].items():
                raw("%s.%s.%s" % (name, form, label), call, p, n)
            raw("%s.%s.%s NULL and %s" % (name, form, first, zero_label), call, dict(p, **{first: None}), zero)
            raw("%s.%s.%s and %s NULL" % (name, form, first, second), call, dict(p, **{first: None, second: None}), r["valid"])

        def device_cases(via, go):                                          # the device form's own refusals, through both
            for k in r["args"]:
                go("%s.run_device.%s.%s_dev + 4" % (name, via, k), dict(dp, **{k: dp[k] + 4}), r["valid"])
            go("%s.run_device.%s.%s NULL and %s_dev + 4" % (name, via, second, first), dict(dp, **{first: dp[first] + 4, second: None}), r["valid"])
            go("%s.run_device.%s.%s and %s_dev + 4" % (name, via, zero_label, first), dict(dp, **{first: dp[first] + 4}), zero)
            go("%s.run_device.%s.every _dev + 4" % (name, via), {k: v + 4 for k, v in dp.items()}, r["valid"])

        device_cases("raw", lambda label, p, n: raw(label, lambda: run_device(o._h, *r["order"](p, n))))
        device_cases("capi", lambda label, p, n: wrapped(label, o.run_device, *r["order"](p, n)))
        for k in r["args"]:
            wrapped("%s.run_device.capi.%s NULL" % (name, k), o.run_device, *r["order"](dict(dp, **{k: 0}), r["valid"]))
        for label, n in r["counts"].items():
            wrapped("%s.run_device.capi.%s" % (name, label), o.run_device, *r["order"](dp, n))
        wrapped("%s.run_device.capi.%s NULL and %s" % (name, first, zero_label), o.run_device, *r["order"](dict(dp, **{first: 0}), zero))
        if name in ("track", "measure", "tracklog"):                        # three sources: a third of 2^31 is too many blocks
            over = (2 ** 31 - 1) // 3 + 1
            raw("%s.run.raw.3 sources n=%d" % (name, over), lambda: run(o3._h, *r["order"](hp, over)))
            raw("%s.run_device.raw.3 sources n=%d" % (name, over), lambda: run_device(o3._h, *r["order"](dp, over)))
            wrapped("%s.run_device.capi.3 sources n=%d" % (name, over), o3.run_device, *r["order"](dp, over))
            raw("%s.run_device.raw.3 sources n=%d and %s_dev + 4" % (name, over, first),
                lambda: run_device(o3._h, *r["order"](dict(dp, **{first: dp[first] + 4}), over)))

    # the host form through capi: no blocks, and the spectrum's two lengths
    wrapped("spectrum.run.capi.frames=0", objs["spectrum"].run, host["wide"], 0)
    wrapped("spectrum.run.capi.frames=2^24+1", objs["spectrum"].run, host["wide"], 2 ** 24 + 1)
    wrapped("spectrum.run.capi.bytes=0", objs["spectrum"].run, np.zeros((SRC, 0), np.uint8), F)
    wrapped("spectrum.run.capi.bytes=a frame short", objs["spectrum"].run, np.zeros((SRC, NB * 2 * N * F - 2 * N), np.uint8), F)
    wrapped("detect.run.capi.n=0", objs["detect"].run, np.zeros((0, N), np.uint32))
    rows0, det0 = np.zeros((SRC, 0), capi.DETECT_ROW), np.zeros((SRC, 0, D), capi.DETECTION)
    slots0, meas0 = np.zeros((SRC, 0, S), capi.TRACK_SLOT), np.zeros((SRC, 0, S), capi.TRACK_MEASURE)
    wrapped("track.run.capi.n=0", objs["track"].run, rows0, det0)
    wrapped("measure.run.capi.n=0", objs["measure"].run, np.zeros((SRC, 0, N), np.uint32), rows0, slots0)
    wrapped("tracklog.run.capi.n=0", objs["tracklog"].run, slots0, meas0)

    # ---- reset and get_state --------------------------------------------------------------------------------------------------
    one, g = np.zeros(S, capi.TRACK_SUMMARY), C.c_uint64()
    for name in ("track", "tracklog"):
        get = getattr(L, "iqd_%s_get_state" % name)
        more = (C.byref(g),) if name == "tracklog" else ()
        raw("%s.reset.raw.object NULL" % name, getattr(L, "iqd_%s_reset" % name), None, untouched=True)
        raw("%s.get_state.raw.object NULL" % name, get, None, 0, capi._np_ptr(one), *more, untouched=True)
        raw("%s.get_state.raw.out NULL" % name, get, objs[name]._h, 0, None, *more)
        raw("%s.get_state.raw.out NULL and source=%d" % (name, SRC), get, objs[name]._h, SRC, None, *more)
        for o, n in ((objs[name], SRC), (objs3[name], 3), (objs[name], 2 ** 32 - 1)):
            raw("%s.get_state.raw.source=%d of %d" % (name, n, o.n_sources), get, o._h, n, capi._np_ptr(one), *more)
        wrapped("%s.get_state.capi.source=%d" % (name, SRC), objs[name].state, SRC)
        wrapped("%s.get_state.capi.source=2^32" % name, objs[name].state, 2 ** 32)
    raw("tracklog.get_state.raw.next_block NULL", L.iqd_tracklog_get_state, objs["tracklog"]._h, 0, capi._np_ptr(one), None)
    raw("tracklog.get_state.raw.next_block NULL and source=%d" % SRC, L.iqd_tracklog_get_state, objs["tracklog"]._h, SRC, capi._np_ptr(one), None)

    stats = eng.stats()
    moved = (stats["device_launches"] - start[0], stats["device_copies"] - start[1])

    # ---- one valid call each, chained on the device arrays --------------------------------------------------------------------
    valid = {}
    for name, r in RUNS.items():
        before = eng.stats()["device_launches"]
        objs[name].run_device(*r["order"](dev, r["valid"]))
        valid[name] = eng.stats()["device_launches"] - before
    eng.synchronize()
    for p in dev.values():
        eng.dev_free(p)
    for o in list(objs.values()) + list(objs3.values()):
        o.close()
    eng.close()
    return dict(table=table, moved=moved, valid=valid)


def dump(table):
    return json.dumps(table, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    from rtlsdrdiags_amd import capi as _capi
    got = collect(_capi)
    assert got["moved"] == (0, 0) and set(got["valid"].values()) == {1}, (got["moved"], got["valid"])
    with open(sys.argv[1], "w") as f:
        f.write(dump(got["table"]))
    print("%d refusals -> %s" % (len(got["table"]), sys.argv[1]))
