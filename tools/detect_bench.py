#!/usr/bin/env python3
"""Band activity detector at size (include/iqdemod.h: iqd_detect_*): 1024 rows - 16 sources x 64 blocks of the standing
16 x 2^20-byte capture - at N = 256, 1024, 2048 (F = 2^13 / N frames per block), behind the iqd_spectrum_run_device call
that produces those rows.  Prints one JSON line and writes it to profiles/detect_bench.json:

    python tools/detect_bench.py [--steps 200] [--settle-ms 300]

  capture        synth.wideband's two stations over noise (one source's 2^19 samples, repeated for the 16 sources)
  spectrum_ms    per N: host clock around iqd_spectrum_run_device + iqd_synchronize, the median of --steps calls after about
                 --settle-ms of the same call untimed (tools/spectrum_bench.py's method)
  detect_ms      the same around iqd_detect_run_device on the rows that call left, with README's parameters (rank N / 2,
                 ratio_q8 2048, guard 1, bridge 8, min width 3, 16 records): most 64-bin words hold no hot bin
  busy_ms        the detector with ratio_q8 256, bridge 0, min width 1, N / 2 records: about half the bins hot, every word
                 walked in full, hundreds of runs per row - the same rows, the other end of what a row can cost
  launch_ms      detect_ms's call on four rows, one workgroup: what a launch and a synchronise cost by themselves
  share, busy_share   detect_ms / spectrum_ms and busy_ms / spectrum_ms of the medians
The four calls of a size alternate three times in the one process and every round's median is listed.  found / busy_found
are n_found summed over the rows, for the record."""
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

    n_src, bps, n_blocks = 16, 1 << 20, 64
    n_rows = n_src * n_blocks
    sizes = [int(v) for v in args.sizes.split(",")]
    eng = capi.Engine(1)
    d_in = eng.dev_alloc(n_src * bps)
    eng.dev_upload(d_in, np.tile(synth.wideband(bps // 2, 2048000.0, STATIONS, seed=7), n_src))
    line = {"workload": "band activity detector, 1024 rows (16 sources x 64 blocks of 2^14 bytes, F = 2^13 / N) behind the "
                        "spectrum call that writes them / two stations over noise / u8",
            "steps": args.steps, "settle_ms": args.settle_ms, "sizes": {}}
    for N in sizes:
        F = bps // n_blocks // (2 * N)
        s = capi.Spectrum(eng, N, n_sources=n_src)
        quiet = capi.Detector(eng, N)
        busy = capi.Detector(eng, N, ratio_q8=256, dc_guard=0, bridge=0, min_width=1, max_detections=N // 2)
        d_pow, d_rows = eng.dev_alloc(n_rows * N * 4), eng.dev_alloc(n_rows * 16)
        d_det = eng.dev_alloc(n_rows * (N // 2) * 32)
        calls = {"spectrum_ms": lambda: s.run_device(d_in, bps, F, d_pow),
                 "detect_ms": lambda: quiet.run_device(d_pow, n_rows, d_rows, d_det),
                 "busy_ms": lambda: busy.run_device(d_pow, n_rows, d_rows, d_det),
                 "launch_ms": lambda: quiet.run_device(d_pow, 4, d_rows, d_det)}
        ms = {k: [] for k in calls}
        found = {}
        for _ in range(3):
            for k, fn in calls.items():
                ms[k].append(round(timed(fn, eng.synchronize, args.steps, args.settle_ms)[0], 4))
                if k in ("detect_ms", "busy_ms"):
                    found[k] = int(eng.dev_download(d_rows, n_rows * 16).view(capi.DETECT_ROW)["n_found"].sum())
        med = {k: float(np.median(v)) for k, v in ms.items()}
        line["sizes"][str(N)] = dict(ms, frames_per_block=F, share=round(med["detect_ms"] / med["spectrum_ms"], 4),
                                     busy_share=round(med["busy_ms"] / med["spectrum_ms"], 4), found=found["detect_ms"],
                                     busy_found=found["busy_ms"])
        for o in (quiet, busy, s):
            o.close()
        for p in (d_pow, d_rows, d_det):
            eng.dev_free(p)
    print(json.dumps(line))
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "detect_bench.json"), "w") as f:
            f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
