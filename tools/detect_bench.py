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
import band_bench_common as bb


def main():
    args = bb.arguments()
    from rtlsdrdiags_amd import capi

    eng = capi.Engine(1)
    d_in = bb.capture(eng)
    line = {"workload": "band activity detector, 1024 rows (16 sources x 64 blocks of 2^14 bytes, F = 2^13 / N) behind the "
                        "spectrum call that writes them / two stations over noise / u8",
            "steps": args.steps, "settle_ms": args.settle_ms, "sizes": {}}
    for N in args.sizes:
        c = bb.Chain(capi, eng, d_in, N, "detect", max_det=N // 2)
        busy = capi.Detector(eng, N, ratio_q8=256, dc_guard=0, bridge=0, min_width=1, max_detections=N // 2)
        calls = {"spectrum_ms": c.spectrum, "detect_ms": c.detect, "busy_ms": lambda: c.detect(detector=busy),
                 "launch_ms": lambda: c.detect(n_rows=4)}
        found = {}

        def after(k):
            if k in ("detect_ms", "busy_ms"):
                found[k] = int(c.download(c.d_rows, bb.N_ROWS * 16, capi.DETECT_ROW)["n_found"].sum())
        ms, med = bb.alternate(calls, eng, args, after)
        line["sizes"][str(N)] = dict(ms, frames_per_block=c.F, share=round(med["detect_ms"] / med["spectrum_ms"], 4),
                                     busy_share=round(med["busy_ms"] / med["spectrum_ms"], 4), found=found["detect_ms"],
                                     busy_found=found["busy_ms"])
        busy.close()
        c.close()
    bb.finish(line, args, "detect_bench.json")
    eng.close()


if __name__ == "__main__":
    main()
