#!/usr/bin/env python3
"""Band track measurements at size (include/iqdemod.h: iqd_measure_*): 16 sources x 64 blocks of the standing 16 x 2^20-byte
capture at N = 256, 1024, 2048 (F = 2^13 / N frames per block), behind the iqd_spectrum_run_device, iqd_detect_run_device and
iqd_track_run_device calls of the same process.  Prints one JSON line and writes it to profiles/measure_bench.json:

    python tools/measure_bench.py [--steps 200] [--settle-ms 300]

  capture        synth.wideband's two stations over noise (one source's 2^19 samples, repeated for the 16 sources)
  track_s8_ms, track_s64_ms       per N: host clock around iqd_track_run_device + iqd_synchronize on the detector's arrays, README's
                 parameters, 8 and 64 slots, the median of --steps calls after about --settle-ms of the same call untimed
                 (tools/track_bench.py's method)
  measure_s8_ms, measure_s64_ms   the same around iqd_measure_run_device on the power rows, the detector's rows and the table that
                 tracker call left, the default thresholds: 1024 workgroups, one per (source, block)
  launch_ms      the 8-slot measurement on one block per source: what a launch and a synchronise cost by themselves
  ratio_to_track measure_s8_ms / track_s8_ms (and _s64) of the same session
The calls of a size alternate three times in the one process and every round's median is listed.  The tracker's state is
carried from one timed call to the next (no reset): after the first call the two stations' tracks are active in every block,
so two slots of every row are measured and the rest are free (with 64 slots: the same two)."""
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
    ap.add_argument("--sizes", default="256,1024,2048")
    ap.add_argument("--no-write", action="store_true", help="print only")
    args = ap.parse_args()
    from chan_bench import timed
    from rtlsdrdiags_amd import capi, synth

    n_src, bps, n_blocks, K = 16, 1 << 20, 64, 16
    n_rows = n_src * n_blocks
    sizes = [int(v) for v in args.sizes.split(",")]
    eng = capi.Engine(1)
    d_in = eng.dev_alloc(n_src * bps)
    eng.dev_upload(d_in, np.tile(synth.wideband(bps // 2, 2048000.0, STATIONS, seed=7), n_src))
    line = {"workload": "band track measurements, 16 sources x 64 blocks of 2^14 bytes (F = 2^13 / N) behind the spectrum, detector "
                        "and tracker calls that feed them / two stations over noise / u8",
            "steps": args.steps, "settle_ms": args.settle_ms, "sizes": {}}
    for N in sizes:
        F = bps // n_blocks // (2 * N)
        s = capi.Spectrum(eng, N, n_sources=n_src)
        det = capi.Detector(eng, N, max_detections=K)
        t = {S: capi.Tracker(eng, N, n_sources=n_src, max_detections=K, n_slots=S) for S in (8, 64)}
        m = {S: capi.Measure(eng, N, n_sources=n_src, n_slots=S) for S in (8, 64)}
        d_pow, d_rows, d_det = eng.dev_alloc(n_rows * N * 4), eng.dev_alloc(n_rows * 16), eng.dev_alloc(n_rows * K * 32)
        d_slots = {S: eng.dev_alloc(n_rows * S * 32) for S in (8, 64)}
        d_meas, d_blocks = eng.dev_alloc(n_rows * 64 * 32), eng.dev_alloc(n_rows * 16)
        s.run_device(d_in, bps, F, d_pow)
        det.run_device(d_pow, n_rows, d_rows, d_det)
        for S in (8, 64):                                         # two calls: from the second on every block has its active tracks
            for _ in range(2):
                t[S].run_device(d_rows, d_det, n_blocks, d_slots[S], d_blocks)
        eng.synchronize()
        calls = {"track_s8_ms": lambda: t[8].run_device(d_rows, d_det, n_blocks, d_slots[8], d_blocks),
                 "measure_s8_ms": lambda: m[8].run_device(d_pow, d_rows, d_slots[8], n_blocks, d_meas),
                 "track_s64_ms": lambda: t[64].run_device(d_rows, d_det, n_blocks, d_slots[64], d_blocks),
                 "measure_s64_ms": lambda: m[64].run_device(d_pow, d_rows, d_slots[64], n_blocks, d_meas),
                 "launch_ms": lambda: m[8].run_device(d_pow, d_rows, d_slots[8], 1, d_meas)}
        ms = {k: [] for k in calls}
        seen = {}
        for _ in range(3):
            for k, fn in calls.items():
                ms[k].append(round(timed(fn, eng.synchronize, args.steps, args.settle_ms)[0], 4))
                if k.startswith("measure"):
                    S = 8 if k == "measure_s8_ms" else 64
                    r = eng.dev_download(d_meas, n_rows * S * 32).view(capi.TRACK_MEASURE)
                    seen[k] = {"measured": int((r["track_id"] != 0).sum()),
                               "hints": [int((r["hint"] == h).sum()) for h in (1, 2, 3)]}
        med = {k: float(np.median(v)) for k, v in ms.items()}
        line["sizes"][str(N)] = dict(ms, frames_per_block=F, records=seen,
                                     ratio_to_track_s8=round(med["measure_s8_ms"] / med["track_s8_ms"], 4),
                                     ratio_to_track_s64=round(med["measure_s64_ms"] / med["track_s64_ms"], 4))
        for o in list(m.values()) + list(t.values()) + [det, s]:
            o.close()
        for p in [d_pow, d_rows, d_det, d_meas, d_blocks] + list(d_slots.values()):
            eng.dev_free(p)
    print(json.dumps(line))
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "measure_bench.json"), "w") as f:
            f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
