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
import band_bench_common as bb


def main():
    args = bb.arguments(sizes=False)
    from rtlsdrdiags_amd import capi

    eng = capi.Engine(1)
    line = {"workload": "band track log, 16 sources x 64 blocks behind the spectrum, detector, tracker and measurement calls that feed "
                        "it / N = 1024, F = 8 / two stations over noise / u8",
            "steps": args.steps, "settle_ms": args.settle_ms}
    c = bb.Chain(capi, eng, bb.capture(eng), 1024, "tracklog")
    calls = {"track_s8_ms": lambda: c.track(8), "log_s8_ms": lambda: c.log(8), "track_s64_ms": lambda: c.track(64),
             "log_s64_ms": lambda: c.log(64), "launch_ms": lambda: c.log(8, n_blocks=1)}
    ms, med = bb.alternate(calls, eng, args)
    seen = {}
    for S in (8, 64):
        st, g = c.lg[S].state(0)
        seen["s%d" % S] = {"live": int((st["track_id"] != 0).sum()), "blocks_seen": int(g), "mode_hints": sorted(int(v) for v in st["mode_hint"] if v)}
    line.update(ms, frames_per_block=c.F, max_events=c.max_events, state=seen,
                ratio_to_track_s8=round(med["log_s8_ms"] / med["track_s8_ms"], 4),
                ratio_to_track_s64=round(med["log_s64_ms"] / med["track_s64_ms"], 4),
                not_measured="hardware counters, a kernel trace, other shapes (more sources, longer calls, calls in which tracks end)")
    c.close()
    bb.finish(line, args, "tracklog_bench.json")
    eng.close()


if __name__ == "__main__":
    main()
