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
import numpy as np

import band_bench_common as bb

I8_MAC_PEAK = 2.5e15


def main():
    args = bb.arguments()
    from rtlsdrdiags_amd import capi, synth

    n_src, bps, M, n_pts, block = bb.N_SRC, bb.BPS, 8, 163, 32768
    eng = capi.Engine(1)
    d_in = eng.dev_alloc(n_src * bps)
    eng.dev_upload(d_in, np.concatenate([synth.white_u8(bps // 2, seed=s) for s in range(n_src)]))
    calls = {}
    for N in args.sizes:
        F = (1 << 17) // N
        s = capi.Spectrum(eng, N, n_sources=n_src)
        d_out = eng.dev_alloc(n_src * (bps // (2 * N * F)) * N * 4)
        calls[N] = (lambda s=s, F=F, d_out=d_out: s.run_device(d_in, bps, F, d_out))
    zs = capi.Channelizer(eng, M, 1, n_src)
    zs.set_survey(offset_hz=[12500.0 * (p - n_pts // 2) for p in range(n_pts)], fs=256000.0 * M, gain_shift=3)
    d_mag = eng.dev_alloc(n_src * (bps // M // block) * n_pts * 4)
    calls["survey"] = lambda: zs.survey_device(d_in, bps, block, d_mag)

    ms, med = bb.alternate(calls, eng, args)
    samples = n_src * bps // 2
    line = {"workload": "band spectrum, 16 sources x 2^20 bytes / blocks of 2^18 bytes (F = 2^17 / N) / default window / u8",
            "steps": args.steps, "settle_ms": args.settle_ms, "survey_ms": ms["survey"], "sizes": {}}
    for N in args.sizes:
        macs = 8 * N * samples
        line["sizes"][str(N)] = {"frames_per_block": (1 << 17) // N, "spectrum_ms": ms[N],
                                 "gsamples_s": round(samples / med[N] / 1e6, 2), "mac_s": float("%.4g" % (macs / (med[N] / 1e3))),
                                 "mfma_share": round(macs / (med[N] / 1e3) / I8_MAC_PEAK, 4),
                                 "over_survey": round(med[N] / med["survey"], 4)}
    bb.finish(line, args, "spectrum_bench.json")
    eng.close()


if __name__ == "__main__":
    main()
