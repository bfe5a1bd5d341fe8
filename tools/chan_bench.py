#!/usr/bin/env python3
"""Wideband channelizer at size (include/iqdemod.h: iqd_channelizer_*): 4096 channels from 16 sources, 2^16 output samples
per channel and call, M = 8, default taps.  Prints one JSON line:

    python tools/chan_bench.py [--steps K] [--settle-ms 100]

  chan_ms            per call, host clock around iqd_channelizer_run_device + synchronize (median of K steps, after
                     about --settle-ms of the same call untimed, like bench.py's clock settle)
  fm_ms / chan_fm_ms FM accept of the channelizer's rows alone (4096 channels x 2^17 bytes) / channelize + FM accept
  bytes, mfma_ops    what one call moves through HBM and issues on the matrix cores, with each as a share of the call's
                     time at 8 TB/s and at 2x the 2.5 PF dense BF16 rate (the i8 rate)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, sync, steps, settle_ms):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < settle_ms / 1e3:
        fn()
        sync()
    ts = []
    for _ in range(steps):
        t = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.mean(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--settle-ms", type=float, default=100.0)
    ap.add_argument("--chan-only", action="store_true", help="only the channelizer calls (counter runs)")
    args = ap.parse_args()
    from rtlsdrdiags_amd import capi

    M, n_src, n_ch, n_out = 8, 16, 4096, 1 << 16
    bps = n_out * 2 * M
    row = bps // M
    rng = np.random.default_rng(1)
    eng = capi.Engine(n_ch)
    eng.set_mode("fm")
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=np.arange(n_ch) % n_src, phase_inc=rng.integers(0, 2 ** 32, n_ch, dtype=np.uint64),
                   gain_shift=np.full(n_ch, 3))
    d_in, d_out = eng.dev_alloc(n_src * bps), eng.dev_alloc(n_ch * row)
    d_pcm, d_cnt = eng.dev_alloc(n_ch * row // 64 * 2), eng.dev_alloc(n_ch * 4)
    from rtlsdrdiags_amd import synth
    eng.dev_upload(d_in, np.concatenate([synth.white_u8(bps // 2, seed=s) for s in range(n_src)]))

    chan = lambda: z.run_device(d_in, bps, d_out)
    chan_ms, chan_mean = timed(chan, eng.synchronize, args.steps, args.settle_ms)
    line = {"workload": "channelizer 4096 ch / 16 sources / 2^16 outputs / M=8 / default taps", "chan_ms": round(chan_ms, 4),
            "chan_mean_ms": round(chan_mean, 4)}
    if not args.chan_only:
        fm = lambda: eng.accept_device(d_out, row, d_pcm, d_cnt)
        both = lambda: (chan(), fm())
        fm_ms, _ = timed(fm, eng.synchronize, args.steps, args.settle_ms)
        both_ms, _ = timed(both, eng.synchronize, args.steps, args.settle_ms)
        line.update(fm_ms=round(fm_ms, 4), chan_fm_ms=round(both_ms, 4))
    K = len(capi.channelizer_default_taps(M))
    nq = (K + 31) // 32
    tiles = n_src * ((n_ch // n_src + 7) // 8)
    mfma = tiles * (n_out // 16) * nq * 2              # v_mfma_i32_16x16x64_i8, two tap planes
    ops = mfma * 16 * 16 * 64 * 2
    hbm = n_src * bps + n_ch * row                     # input once, output rows; taps and phasor stay in cache
    line.update(bytes=hbm, out_bytes=n_ch * row, mfma_instructions=mfma, mfma_ops=ops,
                hbm_bound_ms=round(hbm / 8e12 * 1e3, 4), mfma_bound_ms=round(ops / 5e15 * 1e3, 4),
                hbm_share=round(hbm / 8e12 * 1e3 / chan_ms, 3), mfma_share=round(ops / 5e15 * 1e3 / chan_ms, 3))
    print(json.dumps(line))
    z.close()
    eng.close()


if __name__ == "__main__":
    main()
