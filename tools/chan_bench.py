#!/usr/bin/env python3
"""Wideband channelizer at size (include/iqdemod.h: iqd_channelizer_*): 4096 channels from 16 sources, 2^16 output samples
per channel and call, M = 8, default taps.  Prints one JSON line:

    python tools/chan_bench.py [--steps K] [--settle-ms 100]
    python tools/chan_bench.py --decimation 75 --den 8   (a fractional channelizer: a 2.4 MS/s capture, same outputs)
    python tools/chan_bench.py --format s16            (a signed 16-bit capture, or s8: chz_fmt_kernel; same outputs)
    python tools/chan_bench.py --scan [--steps K]      (scanner-driven channels, written to profiles/ as well)
    python tools/chan_bench.py --survey [--decimation 75 --den 8]   (the band survey against rows of real channels)
    python tools/chan_bench.py --gain [--steps K]      (channels that follow their AGC's IF gain)
    python tools/chan_bench.py --tracks [--steps K]    (channels that follow the slots of a track table)

  chan_ms            per call, host clock around iqd_channelizer_run_device + synchronize (median of K steps, after
                     about --settle-ms of the same call untimed, like bench.py's clock settle)
  fm_ms / chan_fm_ms FM accept of the channelizer's rows alone (4096 channels x 2^17 bytes) / channelize + FM accept
  bytes, mfma_ops    what one call moves through HBM and issues on the matrix cores, with each as a share of the call's
                     time at 8 TB/s and at 2x the 2.5 PF dense BF16 rate (the i8 rate)

--scan: every channel follows its scanner (iqd_channelizer_follow_scanner), FM, squelch and scanning; each call is 4
blocks (block_bytes 32768).  scan_call_ms: iqd_accept_wideband_device + synchronize; fixed_call_ms: the same call with
the channels fixed (chz_kernel); rows_accept_ms: the accept on the rows alone, and walker_ms = scan_call_ms -
rows_accept_ms, an estimate of the walker's share (the two are timed in separate loops).  The walker kernel's own time
comes from a kernel trace of this run: rocprofv3 --kernel-trace (profiles/chan_scan_kernel_trace.json).  The same for 16
following channels (one source), and host_loop_ms: today's host-driven loop for those 16 - one-block calls of
iqd_channelizer_run + iqd_accept_iq with iqd_scanner_get + iqd_channelizer_tuning before each block.

--gain: every channel follows its gain (iqd_channelizer_follow_gain), FM with a running Harris AGC; each call is 4 blocks
(block_bytes 32768), the same size as --scan's.  gain_call_ms: iqd_accept_wideband_device + synchronize; fixed_call_ms:
the same call with the channels fixed (chz_kernel, AGC running open loop); rows_accept_ms and walker_ms as for --scan.

--tracks: every channel follows a slot of a track table (iqd_channelizer_follow_tracks): a synthetic table, S = 64, every
slot active, the increments new in every block, channel c on slot c mod 64 of its source; each call is 4 table blocks
(block_bytes 32768).  tracks_ms: iqd_channelizer_run_device + synchronize (chz_track_kernel and the history kernel: to hold
against --chan-only's chan_ms); tracks_fm_ms: iqd_accept_wideband_device + synchronize with the FM accept behind (against
chan_fm_ms).  host_loop_ms_16: the host-driven loop for 16 followers of one source - per block a slot download,
set_channels with their phase_inc, iqd_channelizer_run of one block, 0x80 over the rows not live, iqd_accept_iq - and
tracks_fm_ms_16, the same 16 channels through the table.

--survey: 16 sources, 2^16 outputs each, a 12.5 kHz grid of 163 points per source (2608 virtual channels), block_bytes
32768.  survey_ms: iqd_channelizer_survey_device + synchronize; grid_run_ms: iqd_channelizer_run_device for 2608 real
channels on the same grid - the cheapest other way to the same bytes, before any accept.  The two alternate three times in
the one process; the medians of each round are listed, and survey_over_grid_run is the ratio of their medians
(profiles/chan_survey_bench.json keeps one session's lines beside the parent build's: DESIGN 4.10.3)."""
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
    ap.add_argument("--scan", action="store_true", help="scanner-driven channels (see above)")
    ap.add_argument("--gain", action="store_true", help="gain-following channels (see above)")
    ap.add_argument("--tracks", action="store_true", help="track-following channels (see above)")
    ap.add_argument("--survey", action="store_true", help="the band survey against run_device on the same grid (see above)")
    ap.add_argument("--grid-only", action="store_true", help="with --survey: only grid_run_ms (a build without the survey)")
    ap.add_argument("--decimation", type=int, default=8, help="M, or P of a fractional decimation P / Q")
    ap.add_argument("--den", type=int, default=1, help="Q of a fractional decimation (1, 2, 4, 8)")
    ap.add_argument("--format", choices=["u8", "s8", "s16"], default="u8", help="the captures' sample format")
    args = ap.parse_args()
    from rtlsdrdiags_amd import capi
    if args.scan:
        return scan_bench(capi, args)
    if args.survey:
        return survey_bench(capi, args)
    if args.gain:
        return gain_bench(capi, args)
    if args.tracks:
        return tracks_bench(capi, args)

    M, Q, n_src, n_ch, n_out = args.decimation, args.den, 16, 4096, 1 << 16
    B = 2 if args.format == "s16" else 1               # bytes per rail (white bytes are full-scale in every format)
    bps = n_out * 2 * M * B // Q
    row = 2 * n_out
    rng = np.random.default_rng(1)
    eng = capi.Engine(n_ch)
    eng.set_mode("fm")
    z = capi.Channelizer(eng, M, n_ch, n_src, decimation_den=Q, sample_format=args.format)
    z.set_channels(0, source=np.arange(n_ch) % n_src, phase_inc=rng.integers(0, 2 ** 32, n_ch, dtype=np.uint64),
                   gain_shift=np.full(n_ch, 3))
    d_in, d_out = eng.dev_alloc(n_src * bps), eng.dev_alloc(n_ch * row)
    d_pcm, d_cnt = eng.dev_alloc(n_ch * row // 64 * 2), eng.dev_alloc(n_ch * 4)
    from rtlsdrdiags_amd import synth
    eng.dev_upload(d_in, np.concatenate([synth.white_u8(bps // 2, seed=s) for s in range(n_src)]))

    chan = lambda: z.run_device(d_in, bps, d_out)
    chan_ms, chan_mean = timed(chan, eng.synchronize, args.steps, args.settle_ms)
    line = {"workload": "channelizer 4096 ch / 16 sources / 2^16 outputs / M=%s / default taps" % (M if Q == 1 else "%d/%d" % (M, Q)),
            "format": args.format, "chan_ms": round(chan_ms, 4),
            "chan_mean_ms": round(chan_mean, 4)}
    if not args.chan_only:
        fm = lambda: eng.accept_device(d_out, row, d_pcm, d_cnt)
        both = lambda: (chan(), fm())
        fm_ms, _ = timed(fm, eng.synchronize, args.steps, args.settle_ms)
        both_ms, _ = timed(both, eng.synchronize, args.steps, args.settle_ms)
        line.update(fm_ms=round(fm_ms, 4), chan_fm_ms=round(both_ms, 4))
    K = -(-len(capi.channelizer_default_taps(M, Q)) // Q)     # taps per branch
    nq = (K + 31) // 32
    tiles = n_src * ((n_ch // n_src + 7) // 8)
    mfma = tiles * (n_out // 16) * nq * 2 * B          # v_mfma_i32_16x16x64_i8, two tap planes x B sample planes
    ops = mfma * 16 * 16 * 64 * 2
    hbm = n_src * bps + n_ch * row                     # input once, output rows; taps and phasor stay in cache
    line.update(bytes=hbm, out_bytes=n_ch * row, mfma_instructions=mfma, mfma_ops=ops,
                hbm_bound_ms=round(hbm / 8e12 * 1e3, 4), mfma_bound_ms=round(ops / 5e15 * 1e3, 4),
                hbm_share=round(hbm / 8e12 * 1e3 / chan_ms, 3), mfma_share=round(ops / 5e15 * 1e3 / chan_ms, 3))
    print(json.dumps(line))
    z.close()
    eng.close()


def survey_bench(capi, args):
    from rtlsdrdiags_amd import synth
    M, Q, n_src, n_out, n_pts, bb = args.decimation, args.den, 16, 1 << 16, 163, 32768
    fs = 256000.0 * M / Q
    bps, row = n_out * 2 * M // Q, 2 * n_out
    offs = [12500.0 * (p - n_pts // 2) for p in range(n_pts)]
    eng = capi.Engine(1)
    d_in = eng.dev_alloc(n_src * bps)
    eng.dev_upload(d_in, np.concatenate([synth.white_u8(bps // 2, seed=s) for s in range(n_src)]))
    zg = capi.Channelizer(eng, M, n_src * n_pts, n_src, decimation_den=Q)
    zg.set_channels(0, source=np.repeat(np.arange(n_src), n_pts), offset_hz=offs * n_src, fs=fs,
                    gain_shift=np.full(n_src * n_pts, 3))
    d_out = eng.dev_alloc(n_src * n_pts * row)
    grid = lambda: zg.run_device(d_in, bps, d_out)
    survey = None
    if not args.grid_only:
        zs = capi.Channelizer(eng, M, 1, n_src, decimation_den=Q)
        zs.set_survey(offset_hz=offs, fs=fs, gain_shift=3)
        d_mag = eng.dev_alloc(n_src * (row // bb) * n_pts * 4)
        survey = lambda: zs.survey_device(d_in, bps, bb, d_mag)
    g, s = [], []
    for _ in range(3):
        g.append(round(timed(grid, eng.synchronize, args.steps, args.settle_ms)[0], 4))
        if survey:
            s.append(round(timed(survey, eng.synchronize, args.steps, args.settle_ms)[0], 4))
    line = {"workload": "band survey, 16 sources / 2^16 outputs / %d points on a 12.5 kHz grid / M=%s / block_bytes %d"
                        % (n_pts, M if Q == 1 else "%d/%d" % (M, Q), bb),
            "grid_run_ms": g, "grid_run_rows_bytes": n_src * n_pts * row}
    if survey:
        line.update(survey_ms=s, survey_over_grid_run=round(float(np.median(s)) / float(np.median(g)), 4))
    print(json.dumps(line))
    eng.close()


def _scan_setup(capi, n_ch, n_src, M, n_out, follow=True):
    from rtlsdrdiags_amd import synth
    bps = n_out * 2 * M
    row = bps // M
    eng = capi.Engine(n_ch)
    eng.set_mode("fm")
    eng.set_squelch(-40)
    centre = 1_700_000_000
    fs = 256000 * M
    eng.scanner_set_parameters(centre - fs // 2, centre + fs // 2 - 64000, 25000)
    eng.scanner_start(True)
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=np.arange(n_ch) % n_src, gain_shift=np.full(n_ch, 3))
    z.set_source_frequency([centre] * n_src)
    z.follow_scanner(follow)
    d_in, d_rows = eng.dev_alloc(n_src * bps), eng.dev_alloc(n_ch * row)
    d_pcm, d_cnt = eng.dev_alloc(n_ch * row // 64 * 2), eng.dev_alloc(n_ch * 4)
    eng.dev_upload(d_in, np.concatenate([synth.white_u8(bps // 2, seed=s) for s in range(n_src)]))
    call = lambda: eng.accept_wideband_device(z, d_in, bps, d_rows, d_pcm, d_cnt)
    rows = lambda: eng.accept_device(d_rows, row, d_pcm, d_cnt)
    return eng, z, call, rows, bps


def scan_bench(capi, args):
    M, n_out = 8, 1 << 16
    line = {"workload": "scanner-driven channelizer, M=8 / default taps / 2^16 outputs (4 blocks) per call"}
    for n_ch, n_src, tag in ((4096, 16, ""), (16, 1, "_16")):
        eng, z, call, rows, _ = _scan_setup(capi, n_ch, n_src, M, n_out)
        scan_ms, _ = timed(call, eng.synchronize, args.steps, args.settle_ms)
        rows_ms, _ = timed(rows, eng.synchronize, args.steps, args.settle_ms)
        z.close(); eng.close()
        eng, z, call, _, _ = _scan_setup(capi, n_ch, n_src, M, n_out, follow=False)
        fixed_ms, _ = timed(call, eng.synchronize, args.steps, args.settle_ms)
        z.close(); eng.close()
        line.update({"scan_call_ms" + tag: round(scan_ms, 4), "rows_accept_ms" + tag: round(rows_ms, 4),
                     "walker_ms" + tag: round(scan_ms - rows_ms, 4), "fixed_call_ms" + tag: round(fixed_ms, 4)})
    # today's host-driven loop for the 16 channels: one block per call, retuned from the scanners between blocks
    from rtlsdrdiags_amd import synth
    n_ch, bb = 16, 32768
    blk_bytes = bb * M
    wide = synth.white_u8(n_out * M, seed=0).reshape(1, -1)
    eng = capi.Engine(n_ch)
    eng.set_mode("fm")
    eng.set_squelch(-40)
    centre, fs = 1_700_000_000, 256000 * M
    eng.scanner_set_parameters(centre - fs // 2, centre + fs // 2 - 64000, 25000)
    eng.scanner_start(True)
    z = capi.Channelizer(eng, M, n_ch, 1)
    z.set_channels(0, gain_shift=np.full(n_ch, 3))

    def loop():
        for b in range(wide.shape[1] // blk_bytes):
            incs, silent = [], []
            for c in range(n_ch):
                d = capi.channelizer_tuning(M, centre, eng.scanner_tuned(c)[0], 1)
                incs.append(0 if d is None else d)
                silent.append(d is None)
            z.set_channels(0, phase_inc=incs)
            r = z.run(wide[:, b * blk_bytes:(b + 1) * blk_bytes])
            r[np.array(silent)] = 0x80
            eng.accept(r)
    loop_ms, _ = timed(loop, eng.synchronize, max(5, args.steps // 5), args.settle_ms)
    z.close(); eng.close()
    line["host_loop_ms_16"] = round(loop_ms, 4)
    print(json.dumps(line))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "chan_scan_bench.json"), "w") as f:
        f.write(json.dumps(line) + "\n")


def _gain_setup(capi, n_ch, n_src, M, n_out, follow=True):
    from rtlsdrdiags_amd import synth
    bps = n_out * 2 * M
    row = bps // M
    eng = capi.Engine(n_ch)
    eng.set_mode("fm")
    eng.set_squelch(-40)
    eng.agc_set_type(1)
    eng.agc_enable(True)
    rng = np.random.default_rng(1)
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=np.arange(n_ch) % n_src, phase_inc=rng.integers(0, 2 ** 32, n_ch, dtype=np.uint64),
                   gain_shift=np.full(n_ch, 3))
    if follow:
        z.follow_gain(True)
    d_in, d_rows = eng.dev_alloc(n_src * bps), eng.dev_alloc(n_ch * row)
    d_pcm, d_cnt = eng.dev_alloc(n_ch * row // 64 * 2), eng.dev_alloc(n_ch * 4)
    eng.dev_upload(d_in, np.concatenate([synth.white_u8(bps // 2, seed=s) for s in range(n_src)]))
    call = lambda: eng.accept_wideband_device(z, d_in, bps, d_rows, d_pcm, d_cnt)
    rows = lambda: eng.accept_device(d_rows, row, d_pcm, d_cnt)
    return eng, z, call, rows


def gain_bench(capi, args):
    M, n_out, n_ch, n_src = 8, 1 << 16, 4096, 16
    line = {"workload": "gain-following channelizer, 4096 ch / 16 sources / M=8 / default taps / 2^16 outputs (4 blocks) per "
                        "call / FM + Harris AGC"}
    eng, z, call, rows = _gain_setup(capi, n_ch, n_src, M, n_out)
    gain_ms, _ = timed(call, eng.synchronize, args.steps, args.settle_ms)
    rows_ms, _ = timed(rows, eng.synchronize, args.steps, args.settle_ms)
    z.close(); eng.close()
    eng, z, call, _ = _gain_setup(capi, n_ch, n_src, M, n_out, follow=False)
    fixed_ms, _ = timed(call, eng.synchronize, args.steps, args.settle_ms)
    z.close(); eng.close()
    line.update(gain_call_ms=round(gain_ms, 4), rows_accept_ms=round(rows_ms, 4), walker_ms=round(gain_ms - rows_ms, 4),
                fixed_call_ms=round(fixed_ms, 4))
    print(json.dumps(line))


def _tracks_setup(capi, n_ch, n_src, M, n_out, nblk=4, S=64):
    from rtlsdrdiags_amd import synth
    bps = n_out * 2 * M
    row = bps // M
    eng = capi.Engine(n_ch)
    eng.set_mode("fm")
    rng = np.random.default_rng(1)
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=np.arange(n_ch) % n_src, gain_shift=np.full(n_ch, 3))
    table = np.zeros((n_src, nblk, S), capi.TRACK_SLOT)     # the kernel cannot tell it from a tracker's output
    table["track_id"] = np.arange(1, S + 1)
    table["state"] = 2
    table["phase_inc"] = rng.integers(0, 2 ** 32, table.shape, dtype=np.uint64)
    d_tab = eng.dev_alloc(table.nbytes)
    eng.dev_upload(d_tab, table.view(np.uint8).reshape(-1))
    z.follow_tracks(np.arange(n_ch) % S)
    z.set_track_table(d_tab, S, nblk, row // nblk, 0, 2)
    d_in, d_rows = eng.dev_alloc(n_src * bps), eng.dev_alloc(n_ch * row)
    d_pcm, d_cnt = eng.dev_alloc(n_ch * row // 64 * 2), eng.dev_alloc(n_ch * 4)
    eng.dev_upload(d_in, np.concatenate([synth.white_u8(bps // 2, seed=s) for s in range(n_src)]))
    run = lambda: z.run_device(d_in, bps, d_rows)
    call = lambda: eng.accept_wideband_device(z, d_in, bps, d_rows, d_pcm, d_cnt)
    return eng, z, run, call, (table, d_tab)


def tracks_bench(capi, args):
    from rtlsdrdiags_amd import synth
    M, n_out, nblk = 8, 1 << 16, 4
    line = {"workload": "track-following channelizer, 4096 ch / 16 sources / M=8 / default taps / 2^16 outputs (4 table blocks) "
                        "per call / S=64, every slot active"}
    eng, z, run, call, _ = _tracks_setup(capi, 4096, 16, M, n_out)
    t, f = [], []
    for _ in range(3):
        t.append(round(timed(run, eng.synchronize, args.steps, args.settle_ms)[0], 4))
        f.append(round(timed(call, eng.synchronize, args.steps, args.settle_ms)[0], 4))
    z.close(); eng.close()
    line.update(tracks_ms=t, tracks_fm_ms=f)
    # 16 followers of one source: through the table, and the host-driven loop of one-block calls
    eng, z, run, call, (table, d_tab) = _tracks_setup(capi, 16, 1, M, n_out)
    line["tracks_fm_ms_16"] = round(timed(call, eng.synchronize, args.steps, args.settle_ms)[0], 4)
    z.follow_tracks(None)
    wide = synth.white_u8(n_out * M, seed=0).reshape(1, -1)
    blk_bytes = wide.shape[1] // nblk

    def loop():
        for b in range(nblk):
            slots = eng.dev_download(d_tab, table.nbytes).view(capi.TRACK_SLOT).reshape(table.shape)[0, b, :16]
            z.set_channels(0, phase_inc=slots["phase_inc"])
            r = z.run(wide[:, b * blk_bytes:(b + 1) * blk_bytes])
            r[slots["state"] < 2] = 0x80
            eng.accept(r)
    line["host_loop_ms_16"] = round(timed(loop, eng.synchronize, max(5, args.steps // 5), args.settle_ms)[0], 4)
    z.close(); eng.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
