#!/usr/bin/env python3
"""PCM tone bank at size (include/iqdemod_tones.h: iqd_tones_*): 4096 channels x 2048 PCM samples per call, the rows and counts
one 4096 x 2^16-sample FM accept of the same process leaves on the device.  Prints one JSON line and writes it to
profiles/tones_bench.json:

    python tools/tones_bench.py [--steps 200] [--settle-ms 300]

  accept_ms          host clock around iqd_accept_iq_device (FM, 4096 channels x 131072 bytes) + iqd_synchronize: the call that
                     produces the rows; the median of --steps calls after about --settle-ms of the same call untimed
                     (tools/chan_bench.py's method)
  l4096_t50_ms       the same around iqd_tones_run_device on those rows: the 50 CTCSS tones, L = 4096 - half a frame per call,
                     so every call carries, and every second one completes 4096 frames (the median lies between the two
                     kinds; both are in l4096_t50_kinds_ms: [calls that complete no frame, calls that complete one])
  l256_t50_ms        L = 256: eight frames per channel and call
  l4096_t64_ms       64 tones
  l4096_t50_nopower_ms   power_dev = NULL
  launch_ms          a bank of 16 channels, L = 32, on 32 samples: what two launches and a synchronise cost by themselves
The calls alternate three times in the one process and every round's median is listed."""
import numpy as np

import band_bench_common as bb

N_CH, N_PCM = 4096, 2048


def main():
    args = bb.arguments(sizes=False)
    from chan_bench import timed
    from rtlsdrdiags_amd import tones

    eng, d_iq, d_pcm, d_cnt, accept = bb.fm_accept_rig(N_CH, n_pcm=N_PCM)
    ctcss = [tones.phase_inc(f, 8000) for f in tones.ctcss_mhz()]
    rng = np.random.default_rng(1)
    banks = {"l4096_t50_ms": (4096, ctcss, True), "l256_t50_ms": (256, ctcss, True),
             "l4096_t64_ms": (4096, ctcss + [int(v) for v in rng.integers(0, 2 ** 32, 14)], True),
             "l4096_t50_nopower_ms": (4096, ctcss, False)}
    objs, arrays, calls = {}, [d_iq, d_pcm, d_cnt], {"accept_ms": accept}
    for key, (L, incs, power) in banks.items():
        t = objs[key] = tones.Tones(eng, N_CH, np.array(incs, np.uint32), frame_len=L, **{k: v for k, v in tones.CTCSS_DEFAULTS.items() if k != "frame_len"})
        F = t.max_frames(N_PCM)
        d = [eng.dev_alloc(N_CH * 4), eng.dev_alloc(N_CH * F * 40), eng.dev_alloc(N_CH * F * len(incs) * 8) if power else 0]
        arrays += [p for p in d if p]
        calls[key] = (lambda t=t, d=d: t.run_device(d_pcm, N_PCM, N_PCM, d[0], d[1], power_dev=d[2], count_dev=d_cnt))
    small = objs["launch_ms"] = tones.Tones(eng, 16, np.array(ctcss[:1], np.uint32), frame_len=32)
    d_small = [eng.dev_alloc(64), eng.dev_alloc(16 * 40)]
    arrays += d_small
    calls["launch_ms"] = lambda: small.run_device(d_pcm, 32, 32, d_small[0], d_small[1])

    ms, med = bb.alternate(calls, eng, args)
    # the two kinds of call at L = 4096, apart: the state alternates, so every second call is of one kind
    kinds = [[], []]
    t = objs["l4096_t50_ms"]
    t.reset()
    for i in range(2 * args.steps):
        kinds[i % 2].append(timed(calls["l4096_t50_ms"], eng.synchronize, 1, 0.0)[0])
    line = dict(workload="PCM tone bank, 4096 channels x 2048 samples per call behind the FM accept (4096 x 2^16 samples) that writes them / "
                         "50 CTCSS tones unless said / default window", steps=args.steps, settle_ms=args.settle_ms, **ms)
    line["l4096_t50_kinds_ms"] = [round(float(np.median(k)), 4) for k in kinds]
    line["ratio_to_accept"] = {k: round(v / med["accept_ms"], 4) for k, v in med.items() if k != "accept_ms"}
    nf = eng.dev_download(arrays[3], N_CH * 4, np.uint32)
    line["frames_last_call_l4096"] = int(nf.sum())
    bb.finish(line, args, "tones_bench.json")
    for o in objs.values():
        o.close()
    for p in arrays:
        eng.dev_free(p)
    eng.close()


if __name__ == "__main__":
    main()
