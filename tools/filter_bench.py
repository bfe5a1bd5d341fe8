#!/usr/bin/env python
"""Times the stand-alone filters (iqd_filter_*, include/iqdemod.h) at size on one MI355X; one JSON line per kind, printed
and appended to profiles/filter_bench.json.

    python tools/filter_bench.py [--steps K] [--settle-ms 100] [--only decimate_i16_audio40,...] [--no-append]

  ms / mean_ms       median / mean of K device-form calls, host clock around iqd_filter_run_device + iqd_synchronize, after
                     about --settle-ms of the same call untimed (tools/chan_bench.py's way)
  samples_per_s      input samples per second
  bytes              what the call must move through HBM: every input sample read once, every output written once (the
                     FIR history and the IIR state are noise at these sizes); frac_of_8TBps: bytes / ms against 8 TB/s
  oracle_*           (a) the same work on ONE host core through oracle/libiqd_oracle.so, measured on oracle_channels rows
                     of the same length and scaled to all of them (the rows are independent); speedup_vs_one_core
  resampler_*        (b) decimators only: this build's iqd_resampler decimate_f32 at the same n_ch, n_in, L and factor -
                     the one older kernel of the same shape; float samples, so it moves twice the bytes

No time here is a pass / fail condition."""
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


def device_rows(eng, rows, n_ch):
    """[n_ch][n_in] on the device: the given rows repeated (iqd_dev_tile)"""
    rows = np.ascontiguousarray(rows)
    total = rows.nbytes // rows.shape[0] * n_ch
    assert rows.nbytes % 16 == 0 and total % rows.nbytes == 0
    d = eng.dev_alloc(total)
    eng.dev_upload(d, rows)
    if total > rows.nbytes:
        eng.dev_tile(d, rows.nbytes, total)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--settle-ms", type=float, default=100.0)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-append", action="store_true")
    ap.add_argument("--oracle-channels", type=int, default=4)
    args = ap.parse_args()
    from oracle import bindings
    from rtlsdrdiags_amd import capi
    O = bindings.Oracle()
    rng = np.random.default_rng(7)
    b_dc, a_dc = np.float32([1.0, -1.0]), np.float32([-0.95])
    work = [  # name, kind, num, den, factor, n_ch, n_in
        ("decimate_i16_audio40", "decimate_i16", O.taps_f32("audio40"), None, 2, 4096, 1 << 16),
        ("decimate_i16_wbfm_d1", "decimate_i16", O.taps_f32("wbfm_d1"), None, 4, 4096, 1 << 16),
        ("fir_i16_hilbert", "fir_i16", O.taps_f32("ssb_hilbert"), None, 1, 4096, 1 << 16),
        ("fir_f32_L48", "fir_f32", rng.normal(0, 0.2, 48).astype(np.float32), None, 1, 4096, 1 << 16),
        ("iir_f32_dcblock", "iir_f32", b_dc, a_dc, 1, 16384, 1 << 14),
        ("iir_f32_order_8_8", "iir_f32", rng.normal(0, 0.1, 8).astype(np.float32), rng.normal(0, 0.05, 8).astype(np.float32), 1,
         16384, 1 << 14),
    ]
    only = [w for w in args.only.split(",") if w]
    eng = capi.Engine(1)
    lines = []
    for name, kind, num, den, factor, n_ch, n_in in work:
        if only and name not in only:
            continue
        i16 = kind in ("decimate_i16", "fir_i16")
        dt = np.int16 if i16 else np.float32
        base = (rng.integers(-32768, 32768, (64, n_in)).astype(np.int16) if i16
                else rng.normal(0, 3000, (64, n_in)).astype(np.float32))
        f = capi.Filter(eng, kind, num, den, factor, n_ch)
        n_out = f.out_count(n_in) if kind != "decimate_i16" else n_in // factor
        d_in = device_rows(eng, base, n_ch)
        d_out = eng.dev_alloc(n_ch * max(n_out, 1) * dt().itemsize)
        call = lambda: f.run_device(d_in, n_in, d_out)
        ms, mean = timed(call, eng.synchronize, args.steps, args.settle_ms)
        nbytes = n_ch * (n_in + n_out) * dt().itemsize
        line = {"bench": "filter", "name": name, "kind": kind, "n_ch": n_ch, "n_in": n_in, "n_taps": len(num),
                "n_den": 0 if den is None else len(den), "factor": factor,
                "clamp_free_taps": capi.filter_clamp_free_taps(num) if i16 else None,
                "ms": round(ms, 4), "mean_ms": round(mean, 4), "samples_per_s": round(n_ch * n_in / (ms / 1e3), 1),
                "bytes": nbytes, "frac_of_8TBps": round(nbytes / (ms / 1e3) / 8e12, 4)}
        # (a) one host core, the oracle, on a few of the rows
        k = max(1, min(args.oracle_channels, 64))
        t = time.perf_counter()
        for c in range(k):
            if kind == "decimate_i16":
                O.decimate_q15(num, factor, base[c])
            elif kind == "fir_i16":
                O.decimate_q15(num, 1, base[c])
            elif kind == "fir_f32":
                O.decimate_f32(num, 1, base[c])
            elif len(num) <= 8 and len(den) <= 4:
                O.iir_f32(num, den, base[c])
            else:
                k = 0
                break
        if k:
            one = 1e3 * (time.perf_counter() - t) / k * n_ch
            line.update(oracle_channels=k, oracle_one_core_ms=round(one, 1), speedup_vs_one_core=round(one / ms, 1))
        else:
            line.update(oracle_channels=0, oracle_note="the oracle's IIR holds 8 and 4 coefficients: no host figure")
        # (b) the float decimator of the resampler family at the same shape
        if kind == "decimate_i16":
            r = capi.Resampler(eng, "decimate_f32", num, factor, n_ch)
            basef = base.astype(np.float32)
            d_inf = device_rows(eng, basef, n_ch)
            d_outf = eng.dev_alloc(n_ch * n_out * 4)
            L = eng._L
            import ctypes as C
            rcall = lambda: eng._check(L.iqd_resampler_run_device(r._h, C.c_void_p(d_inf), n_in, C.c_void_p(d_outf)))
            rms, rmean = timed(rcall, eng.synchronize, args.steps, args.settle_ms)
            line.update(resampler_decimate_f32_ms=round(rms, 4), resampler_decimate_f32_mean_ms=round(rmean, 4),
                        resampler_bytes=n_ch * (n_in + n_out) * 4, resampler_over_filter=round(rms / ms, 3))
            r.close()
            eng.dev_free(d_inf)
            eng.dev_free(d_outf)
        f.close()
        eng.dev_free(d_in)
        eng.dev_free(d_out)
        print(json.dumps(line), flush=True)
        lines.append(line)
    eng.close()
    if lines and not args.no_append:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "filter_bench.json"), "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
