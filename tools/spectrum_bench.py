#!/usr/bin/env python3
"""Band spectrum at size (include/iqdemod.h: iqd_spectrum_*): 16 sources x 2^20 bytes - the standing channelizer capture -
with N = 256, 1024, 2048 and F = 2^17 / N, i.e. blocks of 2^18 bytes (the survey bench's block at M = 8).  Prints one JSON
line and writes it to profiles/spectrum_bench.json:

    python tools/spectrum_bench.py [--steps 200] [--settle-ms 300]

  spectrum_ms    per N: host clock around iqd_spectrum_run_device + iqd_synchronize, the median of --steps calls after about
                 --settle-ms of the same call untimed (tools/chan_bench.py's method); the sizes and the survey alternate
                 three times in the one process and every round's median is listed
  gsamples_s     2^23 samples over the median of the rounds
  mac_s, mfma_share   int8 multiply-accumulates: 8 N per sample (two rails x two coefficient planes x 2 N bytes), and
                 their share of the matrix cores' dense int8 rate, 2.5 x 10^15 MAC/s (twice the 2.5 PF BF16 rate)
  survey_ms      the 163-point survey of tools/chan_bench.py --survey on the same capture (block_bytes 32768: the same
                 2^18 capture bytes per block), and over_survey = spectrum_ms / survey_ms per N"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

I8_MAC_PEAK = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--settle-ms", type=float, default=300.0)
    ap.add_argument("--sizes", default="256,1024,2048")
    ap.add_argument("--no-write", action="store_true", help="print only")
    args = ap.parse_args()
    from chan_bench import timed
    from rtlsdrdiags_amd import capi, synth

    n_src, bps, M, n_pts, bb = 16, 1 << 20, 8, 163, 32768
    sizes = [int(v) for v in args.sizes.split(",")]
    eng = capi.Engine(1)
    d_in = eng.dev_alloc(n_src * bps)
    eng.dev_upload(d_in, np.concatenate([synth.white_u8(bps // 2, seed=s) for s in range(n_src)]))
    calls = {}
    for N in sizes:
        F = (1 << 17) // N
        s = capi.Spectrum(eng, N, n_sources=n_src)
        d_out = eng.dev_alloc(n_src * (bps // (2 * N * F)) * N * 4)
        calls[N] = (lambda s=s, F=F, d_out=d_out: s.run_device(d_in, bps, F, d_out))
    zs = capi.Channelizer(eng, M, 1, n_src)
    zs.set_survey(offset_hz=[12500.0 * (p - n_pts // 2) for p in range(n_pts)], fs=256000.0 * M, gain_shift=3)
    d_mag = eng.dev_alloc(n_src * (bps // M // bb) * n_pts * 4)
    survey = lambda: zs.survey_device(d_in, bps, bb, d_mag)

    ms = {N: [] for N in sizes}
    sv = []
    for _ in range(3):
        for N in sizes:
            ms[N].append(round(timed(calls[N], eng.synchronize, args.steps, args.settle_ms)[0], 4))
        sv.append(round(timed(survey, eng.synchronize, args.steps, args.settle_ms)[0], 4))
    samples = n_src * bps // 2
    sv_med = float(np.median(sv))
    line = {"workload": "band spectrum, 16 sources x 2^20 bytes / blocks of 2^18 bytes (F = 2^17 / N) / default window / u8",
            "steps": args.steps, "settle_ms": args.settle_ms, "survey_ms": sv, "sizes": {}}
    for N in sizes:
        med = float(np.median(ms[N]))
        macs = 8 * N * samples
        line["sizes"][str(N)] = {"frames_per_block": (1 << 17) // N, "spectrum_ms": ms[N],
                                 "gsamples_s": round(samples / med / 1e6, 2), "mac_s": float("%.4g" % (macs / (med / 1e3))),
                                 "mfma_share": round(macs / (med / 1e3) / I8_MAC_PEAK, 4),
                                 "over_survey": round(med / sv_med, 4)}
    print(json.dumps(line))
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "spectrum_bench.json"), "w") as f:
            f.write(json.dumps(line) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
