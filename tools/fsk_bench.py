#!/usr/bin/env python3
"""PCM packet decoder at size (include/iqdemod_fsk.h: iqd_fsk_*): 4096 channels x 2048 PCM samples per call with
iqd_fsk_afsk1200(8000), behind the 4096 x 2^16-sample FM accept of the same process (its counts are the decoder's count_dev).
Prints one JSON line and writes it to profiles/fsk_bench.json:

    python tools/fsk_bench.py [--steps 200] [--settle-ms 300]

  accept_ms        host clock around iqd_accept_iq_device (FM, 4096 channels x 131072 bytes) + iqd_synchronize: the call that
                   produces such rows; the median of --steps calls after about --settle-ms of the same call untimed
                   (tools/chan_bench.py's method)
  tones_l256_ms    the same around iqd_tones_run_device, 50 CTCSS tones at L = 256, on the accept's rows
  afsk_ms          around iqd_fsk_run_device on rows that hold continuous AFSK frames (16-byte payloads between single flags,
                   the same 2048 samples in every call and on every channel, so the frame across the seam is lost)
  silence_ms       on rows of zeros: no transition, no bit set
  noise_ms         on rows of full-scale noise: the most transitions
  fm_rows_ms       on the rows the accept leaves (a 1 kHz tone)
  afsk_nobits_ms   afsk_ms with bits_dev = NULL
  launch_ms        a decoder of 16 channels on 32 samples: what two launches and a synchronise cost by themselves
The calls alternate three times in the one process and every round's median is listed."""
import numpy as np

import band_bench_common as bb

N_CH, N_PCM = 4096, 2048


def afsk_row(phasor, cfg):
    """2048 samples of flags and 16-byte frames (18 with the FCS: above min_len 17), continuous phase, integers only"""
    import sys
    sys.path.insert(0, bb.ROOT)
    from tests import fsk_model as fm
    rng = np.random.default_rng(5)
    bits = fm.hdlc_bits([bytes(rng.integers(0, 256, 16).astype(np.uint8)) for _ in range(4)], 2, 1, 1)
    x = fm.afsk(fm.nrzi_levels(bits), phasor, cfg["mark_inc"], cfg["space_inc"], cfg["baud_inc"], 8000, n=N_PCM)
    assert len(x) == N_PCM
    return x.astype(np.int16)


def main():
    args = bb.arguments(sizes=False)
    from rtlsdrdiags_amd import capi, fsk, tones

    eng, d_iq, d_pcm, d_cnt, accept = bb.fm_accept_rig(N_CH, n_pcm=N_PCM)
    cfg = fsk.afsk1200(8000)
    rows = {"afsk_ms": afsk_row(capi.channelizer_phasor_table(), cfg), "silence_ms": np.zeros(N_PCM, np.int16),
            "noise_ms": np.random.default_rng(6).integers(-32768, 32768, N_PCM).astype(np.int16)}
    objs, arrays, calls = {}, [d_iq, d_pcm, d_cnt], {"accept_ms": accept}

    ctcss = np.array([tones.phase_inc(f, 8000) for f in tones.ctcss_mhz()], np.uint32)
    bank = objs["tones_l256_ms"] = tones.Tones(eng, N_CH, ctcss, frame_len=256, **{k: v for k, v in tones.CTCSS_DEFAULTS.items() if k != "frame_len"})
    d_t = [eng.dev_alloc(N_CH * 4), eng.dev_alloc(N_CH * bank.max_frames(N_PCM) * 40), eng.dev_alloc(N_CH * bank.max_frames(N_PCM) * 50 * 8)]
    arrays += d_t
    calls["tones_l256_ms"] = lambda: bank.run_device(d_pcm, N_PCM, N_PCM, d_t[0], d_t[1], power_dev=d_t[2], count_dev=d_cnt)

    counts = {}
    for key, src, want_bits in [("afsk_ms", "afsk_ms", True), ("silence_ms", "silence_ms", True), ("noise_ms", "noise_ms", True),
                                ("fm_rows_ms", None, True), ("afsk_nobits_ms", "afsk_ms", False)]:
        t = objs[key] = fsk.Fsk(eng, N_CH, **cfg)
        F, Bw, Bc = t.max_frames(N_PCM), t.max_bit_words(N_PCM), t.max_bytes(N_PCM)
        d_rows = d_pcm
        if src:
            d_rows = eng.dev_alloc(N_CH * N_PCM * 2)
            arrays.append(d_rows)
            eng.dev_upload(d_rows, rows[src])
            eng.dev_tile(d_rows, N_PCM * 2, N_CH * N_PCM * 2)
        d = [eng.dev_alloc(N_CH * 4), eng.dev_alloc(N_CH * 4), eng.dev_alloc(N_CH * F * 24), eng.dev_alloc(N_CH * Bc),
             eng.dev_alloc(N_CH * Bw * 4) if want_bits else 0]
        arrays += [p for p in d if p]
        counts[key] = d
        calls[key] = (lambda t=t, d=d, d_rows=d_rows: t.run_device(d_rows, N_PCM, N_PCM, d[0], d[1], d[2], d[3], bits_dev=d[4], count_dev=d_cnt))
    small = objs["launch_ms"] = fsk.Fsk(eng, 16, **cfg)
    d_small = [eng.dev_alloc(64), eng.dev_alloc(64), eng.dev_alloc(16 * 24 * small.max_frames(32)), eng.dev_alloc(16 * small.max_bytes(32))]
    arrays += d_small
    calls["launch_ms"] = lambda: small.run_device(d_pcm, 32, 32, d_small[0], d_small[1], d_small[2], d_small[3])

    ms, med = bb.alternate(calls, eng, args)
    line = dict(workload="PCM packet decoder, afsk1200 at 8 kS/s, 4096 channels x 2048 samples per call / behind the FM accept "
                         "(4096 x 2^16 samples) and beside the tone bank at L = 256 of the same session", steps=args.steps, settle_ms=args.settle_ms, **ms)
    line["ratio_to_accept"] = {k: round(v / med["accept_ms"], 4) for k, v in med.items() if k != "accept_ms"}
    line["ratio_to_tones_l256"] = {k: round(v / med["tones_l256_ms"], 4) for k, v in med.items() if k not in ("accept_ms", "tones_l256_ms")}
    for key in ("afsk_ms", "silence_ms", "noise_ms", "fm_rows_ms"):
        line[key[:-3] + "_last_call"] = dict(bits=int(eng.dev_download(counts[key][0], N_CH * 4, np.uint32).sum()),
                                             frames=int(eng.dev_download(counts[key][1], N_CH * 4, np.uint32).sum()))
    bb.finish(line, args, "fsk_bench.json")
    for o in objs.values():
        o.close()
    for p in arrays:
        eng.dev_free(p)
    eng.close()


if __name__ == "__main__":
    main()
