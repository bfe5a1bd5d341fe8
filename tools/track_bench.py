#!/usr/bin/env python3
"""Band activity tracker at size (include/iqdemod.h: iqd_track_*): 16 sources x 64 blocks of the standing 16 x 2^20-byte
capture at N = 256, 1024, 2048 (F = 2^13 / N frames per block), behind the iqd_spectrum_run_device and iqd_detect_run_device
calls that feed it.  Prints one JSON line and writes it to profiles/track_bench.json:

    python tools/track_bench.py [--steps 200] [--settle-ms 300]

  capture        synth.wideband's two stations over noise (one source's 2^19 samples, repeated for the 16 sources)
  spectrum_ms    per N: host clock around iqd_spectrum_run_device + iqd_synchronize, the median of --steps calls after about
                 --settle-ms of the same call untimed (tools/detect_bench.py's method)
  detect_ms      the same around iqd_detect_run_device on the rows that call left, README's parameters, 16 records
  track_s8_ms, track_s64_ms   the same around iqd_track_run_device on the detector's arrays, README's parameters (gate 512,
                 open 3, hold 2, alpha 64), 8 and 64 slots: 16 waves, each working its source's 64 blocks one after the other
  launch_ms      the 8-slot tracker on one block per source: what a launch and a synchronise cost by themselves
  per_block_us   (track_s8_ms - launch_ms) / 63: what one more block of a source costs the call
The calls of a size alternate three times in the one process and every round's median is listed.  State is carried from
one timed call to the next (no reset): after the first call the two stations' tracks are active and every block matches."""
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
    line = {"workload": "band activity tracker, 16 sources x 64 blocks of 2^14 bytes (F = 2^13 / N) behind the spectrum and "
                        "detector calls that feed it / two stations over noise / u8",
            "steps": args.steps, "settle_ms": args.settle_ms, "sizes": {}}
    for N in sizes:
        F = bps // n_blocks // (2 * N)
        s = capi.Spectrum(eng, N, n_sources=n_src)
        det = capi.Detector(eng, N, max_detections=K)
        t8 = capi.Tracker(eng, N, n_sources=n_src, max_detections=K, n_slots=8)
        t64 = capi.Tracker(eng, N, n_sources=n_src, max_detections=K, n_slots=64)
        d_pow, d_rows, d_det = eng.dev_alloc(n_rows * N * 4), eng.dev_alloc(n_rows * 16), eng.dev_alloc(n_rows * K * 32)
        d_slots, d_blocks = eng.dev_alloc(n_rows * 64 * 32), eng.dev_alloc(n_rows * 16)
        s.run_device(d_in, bps, F, d_pow)
        det.run_device(d_pow, n_rows, d_rows, d_det)
        eng.synchronize()
        # one block per source: the same arrays read as [16][1] rows - the first 16 rows, whatever source they belong to
        calls = {"spectrum_ms": lambda: s.run_device(d_in, bps, F, d_pow),
                 "detect_ms": lambda: det.run_device(d_pow, n_rows, d_rows, d_det),
                 "track_s8_ms": lambda: t8.run_device(d_rows, d_det, n_blocks, d_slots, d_blocks),
                 "track_s64_ms": lambda: t64.run_device(d_rows, d_det, n_blocks, d_slots, d_blocks),
                 "launch_ms": lambda: t8.run_device(d_rows, d_det, 1, d_slots, d_blocks)}
        ms = {k: [] for k in calls}
        live = {}
        for _ in range(3):
            for k, fn in calls.items():
                ms[k].append(round(timed(fn, eng.synchronize, args.steps, args.settle_ms)[0], 4))
                if k.startswith("track"):
                    b = eng.dev_download(d_blocks, n_rows * 16).view(capi.TRACK_BLOCK)
                    live[k] = [int(b["n_active"].sum()), int(b["n_unplaced"].sum())]
        med = {k: float(np.median(v)) for k, v in ms.items()}
        line["sizes"][str(N)] = dict(ms, frames_per_block=F, found=int(eng.dev_download(d_rows, n_rows * 16).view(capi.DETECT_ROW)["n_found"].sum()),
                                     active_unplaced=live, share_of_detect=round(med["track_s8_ms"] / med["detect_ms"], 4),
                                     per_block_us=round(1000.0 * (med["track_s8_ms"] - med["launch_ms"]) / (n_blocks - 1), 4),
                                     per_block_s64_us=round(1000.0 * (med["track_s64_ms"] - med["launch_ms"]) / (n_blocks - 1), 4))
        for o in (t8, t64, det, s):
            o.close()
        for p in (d_pow, d_rows, d_det, d_slots, d_blocks):
            eng.dev_free(p)
    print(json.dumps(line))
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "track_bench.json"), "w") as f:
            f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
