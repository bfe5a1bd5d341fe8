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
import band_bench_common as bb


def main():
    args = bb.arguments()
    from rtlsdrdiags_amd import capi

    eng = capi.Engine(1)
    d_in = bb.capture(eng)
    line = {"workload": "band track measurements, 16 sources x 64 blocks of 2^14 bytes (F = 2^13 / N) behind the spectrum, detector "
                        "and tracker calls that feed them / two stations over noise / u8",
            "steps": args.steps, "settle_ms": args.settle_ms, "sizes": {}}
    for N in args.sizes:
        c = bb.Chain(capi, eng, d_in, N, "measure")
        calls = {"track_s8_ms": lambda: c.track(8), "measure_s8_ms": lambda: c.measure(8), "track_s64_ms": lambda: c.track(64),
                 "measure_s64_ms": lambda: c.measure(64), "launch_ms": lambda: c.measure(8, n_blocks=1)}
        seen = {}

        def after(k):
            if k.startswith("measure"):
                S = 8 if k == "measure_s8_ms" else 64
                r = c.download(c.d_meas[S], bb.N_ROWS * S * 32, capi.TRACK_MEASURE)
                seen[k] = {"measured": int((r["track_id"] != 0).sum()), "hints": [int((r["hint"] == h).sum()) for h in (1, 2, 3)]}
        ms, med = bb.alternate(calls, eng, args, after)
        line["sizes"][str(N)] = dict(ms, frames_per_block=c.F, records=seen,
                                     ratio_to_track_s8=round(med["measure_s8_ms"] / med["track_s8_ms"], 4),
                                     ratio_to_track_s64=round(med["measure_s64_ms"] / med["track_s64_ms"], 4))
        c.close()
    bb.finish(line, args, "measure_bench.json")
    eng.close()


if __name__ == "__main__":
    main()
