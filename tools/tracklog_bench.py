#!/usr/bin/env python3
"""The band track log at size (include/iqdemod.h: iqd_tracklog_*): 16 sources x 64 blocks of the standing 16 x 2^20-byte capture
at N = 1024 (F = 8 frames per block), 8 and 64 slots, behind the iqd_spectrum_run_device, iqd_detect_run_device,
iqd_track_run_device and iqd_measure_run_device calls of the same process.  Prints one JSON line and writes it to
profiles/tracklog_bench.json:

    python tools/tracklog_bench.py [--steps 200] [--settle-ms 300]

  capture        synth.wideband's two stations over noise (one source's 2^19 samples, repeated for the 16 sources)
  track_s8_ms, track_s64_ms   host clock around iqd_track_run_device + iqd_synchronize on the detector's arrays, README's
                 parameters, the median of --steps calls after about --settle-ms of the same call untimed (tools/track_bench.py's
                 method)
  log_s8_ms, log_s64_ms       the same around iqd_tracklog_run_device on the table that tracker call left and the measurement
                 records of that table, the default settings: 16 workgroups of one wave, one per source
  launch_ms      the 8-slot log on one block per source: what a launch and a synchronise cost by themselves
  ratio_to_track log_s8_ms / track_s8_ms (and _s64) of the same session
The calls alternate three times in the one process and every round's median is listed.  The tracker's and the log's state are
carried from one timed call to the next (no reset): the two stations' tracks are active in every block, so two summaries of
every row are live and gather a vote per block, the rest are free, and no track ends (no event is stored; the event list's
256 records per source are zeroed in every call).  No time here is a pass / fail condition."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STATIONS = [{"offset": -700e3, "kind": "fm", "amplitude": 25.0, "tone": 1000.0},
            {"offset": 250e3, "kind": "am", "amplitude": 25.0, "tone": 700.0}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--settle-ms", type=float, default=300.0)
    ap.add_argument("--no-write", action="store_true", help="print only")
    args = ap.parse_args()
    from chan_bench import timed
    from rtlsdrdiags_amd import capi, synth

    n_src, bps, n_blocks, K, N = 16, 1 << 20, 64, 16, 1024
    n_rows = n_src * n_blocks
    F = bps // n_blocks // (2 * N)
    E = capi.tracklog_defaults()["max_events"]
    eng = capi.Engine(1)
    d_in = eng.dev_alloc(n_src * bps)
    eng.dev_upload(d_in, np.tile(synth.wideband(bps // 2, 2048000.0, STATIONS, seed=7), n_src))
    line = {"workload": "band track log, 16 sources x 64 blocks behind the spectrum, detector, tracker and measurement calls that feed "
                        "it / N = 1024, F = 8 / two stations over noise / u8",
            "steps": args.steps, "settle_ms": args.settle_ms}
    s = capi.Spectrum(eng, N, n_sources=n_src)
    det = capi.Detector(eng, N, max_detections=K)
    t = {S: capi.Tracker(eng, N, n_sources=n_src, max_detections=K, n_slots=S) for S in (8, 64)}
    m = {S: capi.Measure(eng, N, n_sources=n_src, n_slots=S) for S in (8, 64)}
    lg = {S: capi.TrackLog(eng, n_sources=n_src, n_slots=S) for S in (8, 64)}
    d_pow, d_rows, d_det = eng.dev_alloc(n_rows * N * 4), eng.dev_alloc(n_rows * 16), eng.dev_alloc(n_rows * K * 32)
    d_slots = {S: eng.dev_alloc(n_rows * S * 32) for S in (8, 64)}
    d_meas = {S: eng.dev_alloc(n_rows * S * 32) for S in (8, 64)}
    d_blocks, d_summary = eng.dev_alloc(n_rows * 16), eng.dev_alloc(n_rows * 64 * 64)
    d_events, d_counts = eng.dev_alloc(n_src * E * 64), eng.dev_alloc(n_src * 16)
    s.run_device(d_in, bps, F, d_pow)
    det.run_device(d_pow, n_rows, d_rows, d_det)
    for S in (8, 64):                                             # two calls: from the second on every block has its active tracks
        for _ in range(2):
            t[S].run_device(d_rows, d_det, n_blocks, d_slots[S], d_blocks)
        m[S].run_device(d_pow, d_rows, d_slots[S], n_blocks, d_meas[S])
    eng.synchronize()
    calls = {"track_s8_ms": lambda: t[8].run_device(d_rows, d_det, n_blocks, d_slots[8], d_blocks),
             "log_s8_ms": lambda: lg[8].run_device(d_slots[8], d_meas[8], n_blocks, d_summary, d_events, d_counts),
             "track_s64_ms": lambda: t[64].run_device(d_rows, d_det, n_blocks, d_slots[64], d_blocks),
             "log_s64_ms": lambda: lg[64].run_device(d_slots[64], d_meas[64], n_blocks, d_summary, d_events, d_counts),
             "launch_ms": lambda: lg[8].run_device(d_slots[8], d_meas[8], 1, d_summary, d_events, d_counts)}
    ms = {k: [] for k in calls}
    for _ in range(3):
        for k, fn in calls.items():
            ms[k].append(round(timed(fn, eng.synchronize, args.steps, args.settle_ms)[0], 4))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    seen = {}
    for S in (8, 64):
        st, g = lg[S].state(0)
        seen["s%d" % S] = {"live": int((st["track_id"] != 0).sum()), "blocks_seen": int(g), "mode_hints": sorted(int(v) for v in st["mode_hint"] if v)}
    line.update(ms, frames_per_block=F, max_events=E, state=seen,
                ratio_to_track_s8=round(med["log_s8_ms"] / med["track_s8_ms"], 4),
                ratio_to_track_s64=round(med["log_s64_ms"] / med["track_s64_ms"], 4),
                not_measured="hardware counters, a kernel trace, other shapes (more sources, longer calls, calls in which tracks end)")
    for o in list(lg.values()) + list(m.values()) + list(t.values()) + [det, s]:
        o.close()
    print(json.dumps(line))
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "tracklog_bench.json"), "w") as f:
            f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
