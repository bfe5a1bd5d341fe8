#!/usr/bin/env python3
"""bench.py — IQ MSamples/s through the demodulator chains on N MI355X GPUs, with the HBM roofline fraction
of the dominant kernel and, with --full, the CPU baseline timed beside it.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config 0|1|2|3|4] [--dump-outputs DIR] [--full]

A plain run sets up, settles the clocks, warms up, times the K steps and prints the line.  Everything else the benchmark
measures - the from-idle figure, the CPU baseline, the PCIe-inclusive host path, the rocprofv3 counter passes, the other
BASELINE configurations as sub-lines and configs[0]'s parity check against the CPU chain - runs only with `--full`.
`--dump-outputs DIR` writes what the timed path returned in its last step as DIR/<name>.npy (float32 / float64).

`python bench.py --gpus N` with N > 1 starts its own ranks (torch.distributed.run as a CHILD process, one rank per GPU
over RCCL) when it was not itself started by a launcher, and relays rank 0's line and the exit code.

Default workload (BASELINE.json configs[1]): WBFM, 1 channel per GPU, 2^28 synthetic IQ samples
(512 MiB of uint8 I/Q) resident in HBM before the timed region.  `--config N` selects BASELINE.json configs[N]:

    0  one FM channel, 2^20 samples from a file through the C++ IqDataProcessor::acceptIqData in 32768-byte blocks
       (the reference's own operating point: one 64 ms block per call; reports us per block beside MS/s)
    1  WBFM, 1 channel x 2^28 samples                                   (the metric's configuration)
    2  FM, 4096 channels x 2^16 samples (256 ms of signal each)
    3  mixed AM/FM/WBFM/LSB/USB, 4096 channels per GPU x 2^16 samples    (32768 channels over 8 GPUs)
    4  LSB+USB, rotation selector varying per channel, Harris AGC running, squelch threshold raised so that blocks
       gate (loud / quiet blocks per channel), 8192 channels per GPU x 2^16 samples  (65536 channels over 8 GPUs)

A "step" is one iqd_accept_iq_device() call over the whole batch: the chain kernel(s), the hand-off verification, the
squelch / AGC bookkeeping and the state update.  With N > 1 every rank runs its own channels on its own GPU
(independent channels are the shard; no data-path collective), so the job is weak-scaled and `value` is the sum over
ranks divided by the slowest rank's time.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import re
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

ALGO_BYTES_PER_SAMPLE = 2.0 + 2.0 / 32.0     # int8 I + int8 Q in, int16 PCM out at 1/32 rate
HBM_PEAK_GBS = 8000.0                        # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
MAX_CLOCK_GHZ = 2.4                          # (same guide: max clock)
METRIC = "IQ MSamples/s through WBFM chain at 1/2/4/8 GPUs; % HBM roofline"

CONFIGS = {
    0: dict(mode="fm", channels=1, log2=20, tag="fm_file",
            what="BASELINE configs[0]: single FM channel, 256 kS/s uint8 IQ from a file through IqDataProcessor::acceptIqData "
                 "in 32768-byte blocks (C++ class over the C ABI; one 64 ms block per call)"),
    1: dict(mode="wbfm", channels=1, log2=28, tag="wbfm_2p28",
            what="BASELINE configs[1]: WBFM, 1 channel, 2^28-sample synthetic IQ"),
    2: dict(mode="fm", channels=4096, log2=16, tag="fm_4096",
            what="BASELINE configs[2]: 4096 concurrent FM channels, 2^16 samples (256 ms at 256 kS/s) each per step"),
    3: dict(mode="mixed", channels=4096, log2=16, tag="mixed_4096",
            what="BASELINE configs[3]: mixed AM/FM/WBFM/LSB/USB (channel % 5), 4096 channels per GPU = 32768 over 8 GPUs, "
                 "2^16 samples each per step"),
    4: dict(mode="ssb_stress", channels=8192, log2=16, tag="ssb_8192",
            what="BASELINE configs[4]: LSB+USB alternating, rotation selector (the reference's only NCO: +Fs/4, none, -Fs/4) "
                 "varying per channel, Harris AGC running, squelch threshold raised so that blocks gate, 8192 channels per GPU = "
                 "65536 over 8 GPUs, 2^16 samples each per step"),
}


# ---- CPU baseline --------------------------------------------------------------------------------------------
def _cpu_chain(kind_mode):
    from oracle import bindings as B
    if B.have_ref():
        chain, kind = B.Reference().chain(), "reference"
    else:
        chain, kind = B.Oracle().chain(), "port"
    chain.set_mode(kind_mode)
    return chain, kind


def _cpu_worker(mode, period_u8, seconds, q, start_at=None):
    """One independent channel on one core for about `seconds`; reports (samples, elapsed)."""
    chain, _ = _cpu_chain(mode)
    piece = period_u8[: 2 << 20]                  # 2^20 samples per call: the clock is read often enough
    chain.accept_stream(piece[: 1 << 18])         # warm the code and the tables
    if start_at is not None:                      # a common start (with every worker's clock starting as it was
        time.sleep(max(0.0, start_at - time.time()))   # forked, the first ran alone and the last beside 255 others: 0.2-0.5 G/s from run to run)
    done, t0 = 0, time.perf_counter()
    while True:
        chain.accept_stream(piece)
        done += len(piece) // 2
        dt = time.perf_counter() - t0
        if dt >= seconds:
            break
    q.put((done, dt))


def host_cores():
    """What this process may really use of the host: hardware threads it is allowed on (affinity), the cgroup's CPU quota
    (cpu.max of cgroup v2, cfs_quota_us / cfs_period_us of v1), physical cores and threads per core as /proc/cpuinfo lists them.
    `cores_effective` = the smaller of affinity and quota: the most cores' worth of time the baseline can get."""
    logical = os.cpu_count() or 1
    affinity = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else logical
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            quota = None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        try:
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                q, per = float(f.read()), float(g.read())
                quota = None if q <= 0 else q / per
        except (OSError, ValueError):
            pass
    physical, tpc = None, None
    try:
        cores, sib = set(), None
        phys = core = None
        with open("/proc/cpuinfo") as f:
            for ln in f:
                k, _, v = ln.partition(":")
                k = k.strip()
                if k == "physical id":
                    phys = v.strip()
                elif k == "core id":
                    core = v.strip()
                    cores.add((phys, core))
                elif k == "siblings" and sib is None:
                    sib = int(v)
                elif k == "cpu cores" and tpc is None and sib:
                    tpc = max(1, sib // max(1, int(v)))
        physical = len(cores) or None
    except (OSError, ValueError):
        pass
    eff = min(affinity, quota) if quota else affinity
    return {"logical": logical, "affinity": affinity, "cgroup_quota_cores": None if quota is None else round(quota, 2),
            "physical_cores": physical, "threads_per_core": tpc, "cores_effective": round(eff, 2)}


def _cpu_level(ctx, cpu_mode, period_u8, n_procs, seconds):
    """n_procs independent channels, one process each, from a common start; (aggregate MS/s, slowest process's seconds)."""
    q = ctx.Queue()
    start_at = time.time() + 0.4 + 0.006 * n_procs        # (forking 256 workers takes about a second)
    procs = [ctx.Process(target=_cpu_worker, args=(cpu_mode, period_u8, seconds, q, start_at)) for _ in range(n_procs)]
    for p in procs:
        p.start()
    got = [q.get() for _ in procs]
    for p in procs:
        p.join()
    return sum(d for d, _ in got) / max(t for _, t in got) / 1e6, max(t for _, t in got)


def cpu_all_cores(cpu_mode, period_u8, kind, one_core_value, seconds_target):
    """The reference on every host core this process may use - as a SERIES over 1, 2, 4, ... processes (one independent channel
    each: the reference is single-threaded per channel, src_diags/DataConsumer.cc:52), so that the knee shows: where the
    aggregate stops following the process count is where the box stops giving cores (a cgroup quota, SMT siblings, memory).
    VERDICT r5 item 7: 256 processes had given ten cores' worth, and the line said "256 cores"."""
    import multiprocessing as mp
    host = host_cores()
    ctx = mp.get_context("fork")
    n_max = host["affinity"]
    levels = sorted({min(n_max, 1 << k) for k in range(0, 12)} | {n_max})
    per_level = max(1.0, min(2.0, 0.8 * seconds_target / len(levels)))
    t0 = time.perf_counter()
    series = []
    for n_procs in levels:
        agg, _ = _cpu_level(ctx, cpu_mode, period_u8, n_procs, per_level)
        if series and agg < series[-1]["value"]:        # more processes, less done: a neighbour's load or a late start - once more
            agg = max(agg, _cpu_level(ctx, cpu_mode, period_u8, n_procs, per_level)[0])
        series.append({"processes": n_procs, "value": round(agg, 3), "per_process": round(agg / n_procs, 3)})
    wall = time.perf_counter() - t0
    best = max(series, key=lambda e: e["value"])
    knee = next(e["processes"] for e in series if e["value"] >= 0.9 * best["value"])
    full = series[-1]
    # `value` = the best level of the series with `cores` = its process count (a box that gives this process a CPU quota of 16
    # cores out of 256 hardware threads does its best work at 16-32 processes, and 256 of them only contend); the figure with one
    # process per hardware thread stays beside it
    return {"value": best["value"], "unit": "MSamples/s", "cores": best["processes"], "kind": kind, "wall_s": round(wall, 2),
            "host": host, "cores_effective": host["cores_effective"],
            "cores_worth": round(best["value"] / one_core_value, 1) if one_core_value else None,
            "at_all_hardware_threads": {"processes": n_max, "value": full["value"]},
            "series": series, "knee_processes": knee,
            "sample": "the best of a series with 1, 2, 4, ... %d processes (up to one per hardware thread this process may run on), one "
                      "independent %s channel each, 2^20-sample calls of the bench signal for %.1f s from a common start; `cores` = the "
                      "processes of that best level; `cores_worth` = value / the one-core figure; `host` = affinity, cgroup quota, physical "
                      "cores as the box reports them" % (n_max, cpu_mode.upper(), per_level)}


def cpu_baseline(period_u8, mode="wbfm", seconds_target=10.0, all_cores=True):
    """The reference CPU chain itself (oracle/_ref: the unmodified reference sources; `kind` says "port" when that
    library is absent and the oracle restatement is timed instead) on a bounded sample of the bench signal: one host
    core, and every host core this process may use with one independent channel per process (the reference is
    single-threaded per channel: src_diags/DataConsumer.cc:52)."""
    cpu_mode = {"mixed": "wbfm", "ssb_stress": "lsb"}.get(mode, mode)
    chain, kind = _cpu_chain(cpu_mode)
    n_period = len(period_u8) // 2
    t0 = time.perf_counter()
    chain.accept_stream(period_u8[: 2 << 21])
    rate = (1 << 21) / (time.perf_counter() - t0)
    reps = max(1, min(64, int(seconds_target * rate / n_period)))
    t0 = time.perf_counter()
    for _ in range(reps):
        chain.accept_stream(period_u8)
    dt = time.perf_counter() - t0
    out = {"value": round(reps * n_period / dt / 1e6, 3), "unit": "MSamples/s", "cores": 1, "kind": kind,
           "sample": "%s, 1 channel, %d x 2^%d samples of the bench signal through IqDataProcessor::acceptIqData in "
                     "32768-byte blocks, 1 thread" % (cpu_mode.upper(), reps, int(np.log2(n_period)))}
    if all_cores:
        out["all_cores"] = cpu_all_cores(cpu_mode, period_u8, kind, out["value"], seconds_target)
    return out


def host_path(eng, iq_dev, n, n_ch, reps=3):
    """The same workload through the host-pointer entry point (iqd_accept_iq): IQ in page-locked host memory,
    uploaded in slices that overlap the kernels, PCM downloaded.  Reported beside `value`, never as it."""
    iq = eng.host_array((n_ch, 2 * n))
    pcm = eng.host_array((n_ch, n // 32), np.int16)
    iq[:] = iq_dev.view(n_ch, -1).cpu().numpy()
    cnt = np.zeros(n_ch, np.uint32)
    eng.accept_into(iq, pcm, cnt)
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.accept_into(iq, pcm, cnt)
    dt = (time.perf_counter() - t0) / reps
    eng.host_free(iq)
    eng.host_free(pcm)
    return {"value": round(n * n_ch / dt / 1e6, 1), "unit": "MSamples/s", "ms_per_step": round(1e3 * dt, 3),
            "GB_per_s_over_pcie": round(2.0625 * n * n_ch / dt / 1e9, 2),
            "what": "iqd_accept_iq from page-locked host buffers (upload, kernels, PCM download), %d calls" % reps}


DUMP_MAX_PCM = 1 << 23          # PCM samples written in full (32 MB as float32); beyond that a fixed, seeded sample of
DUMP_SAMPLE = 1 << 22           # this many (16 MB as float32 + 32 MB of float64 positions: the dump stays under 64 MB)


def dump_outputs(out_dir, torch, pcm, small):
    """--dump-outputs: what a caller of the timed path holds after the last step, as DIR/<name>.npy - `pcm` [channels][row]
    (samples past a channel's count zeroed: they are not part of the result), `pcm_count`, `magnitude` [channels][blocks] and
    `signal_present` [channels][blocks]; `small` is None under --no-magnitude, whose calls return the PCM only.  Exact values:
    int16 / uint8 as float32, int32 / uint32 as float64.  A PCM of more than DUMP_MAX_PCM samples is written as DUMP_SAMPLE
    samples at seeded positions (`pcm` flat, `pcm_index` their flat indices), so that two runs with the same arguments write
    the same files."""
    os.makedirs(out_dir, exist_ok=True)
    n_ch, row = pcm.shape
    if small is not None:
        cnt, mag, allowed = small
        cols = torch.arange(row, device=pcm.device, dtype=torch.int64)
        pcm = torch.where(cols.unsqueeze(0) < cnt.to(torch.int64).unsqueeze(1), pcm, torch.zeros_like(pcm))
        np.save(os.path.join(out_dir, "pcm_count.npy"), cnt.cpu().numpy().astype(np.float64))
        np.save(os.path.join(out_dir, "magnitude.npy"), mag.view(n_ch, -1).cpu().numpy().view(np.uint32).astype(np.float64))
        np.save(os.path.join(out_dir, "signal_present.npy"), allowed.view(n_ch, -1).cpu().numpy().astype(np.float32))
    pcm = pcm.cpu().numpy()
    if pcm.size > DUMP_MAX_PCM:
        idx = np.sort(np.random.default_rng(20240601).choice(pcm.size, DUMP_SAMPLE, replace=False))
        np.save(os.path.join(out_dir, "pcm_index.npy"), idx.astype(np.float64))
        pcm = pcm.reshape(-1)[idx]
    np.save(os.path.join(out_dir, "pcm.npy"), pcm.astype(np.float32))


def profile_summary(tag):
    """Counter-derived figures of the same workload from the committed rocprofv3 summary (profiles/, written by
    tools/profile.sh + tools/pmc_summary.py) - accepted only if it was taken from THESE kernel sources (the summary
    records a hash of rtlsdrdiags_amd/csrc): a kernel change without a new profile must not keep stale counters."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_summary
    now = pmc_summary.source_hash()
    for rnd in (6, 5, 4, 3, 2, 1):
        path = os.path.join(ROOT, "profiles", "r%d_%s_pmc.json" % (rnd, tag))
        if os.path.exists(path):
            with open(path) as f:
                prof = json.load(f)
            if prof.get("sources_sha16") == now:
                return prof, os.path.relpath(path, ROOT)
            return None, "%s is stale (taken from sources %s, running %s)" % (os.path.relpath(path, ROOT), prof.get("sources_sha16"), now)
    return None, None


PMC_PASSES = (("fetch", ["FETCH_SIZE"]), ("write", ["WRITE_SIZE"]), ("sq1", ["SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "GRBM_GUI_ACTIVE"]))


def live_pmc(argv, needle, samples_per_launch, passes=("fetch", "write", "sq1")):
    """HBM traffic and vector-ALU counters of the SAME command, collected now: three short rocprofv3 passes of this
    script as child processes (--pmc on its own, no trace domain beside it, the program itself after `--`, from /tmp:
    MI355X_MICROARCH.md), condensed by tools/pmc_summary.py.  None if rocprofv3 is not there or a pass fails."""
    import shutil
    import subprocess
    import tempfile
    rocprof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not rocprof or not needle:
        return {"skipped": "rocprofv3 is not installed"} if needle else None
    # never a profiler inside a profiler: `rocprofv3 -- python bench.py` preloads its tool library into this process
    under = [k for k in os.environ if k.startswith(("ROCP_", "ROCPROFILER_", "ROCPROF_"))] + \
            [k for k in ("LD_PRELOAD",) if "rocprof" in os.environ.get(k, "")]
    if under:
        return {"skipped": "this run is itself under a profiler (%s): no nested counter passes" % ", ".join(sorted(under)[:3])}
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_summary
    tmp = tempfile.mkdtemp(prefix="iqd_pmc_", dir="/tmp")
    child = [sys.executable, os.path.abspath(__file__)] + [a for a in argv if a not in ("--gather",)] + \
            ["--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-host-path", "--no-live-pmc", "--prewarm-ms", "0", "--no-other-configs"]
    env = dict(os.environ, TMPDIR="/tmp")
    child_ms = None
    try:
        for sub, counters in PMC_PASSES:
            if sub not in passes:
                continue
            r = subprocess.run([rocprof, "--pmc"] + counters + ["--output-format", "csv", "-d", os.path.join(tmp, sub), "--"] + child,
                               cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=240)
            if r.returncode != 0:
                return {"skipped": "the rocprofv3 --pmc %s pass exited with %d" % (" ".join(counters), r.returncode)}
            if sub == "sq1":   # the kernel time of the very pass the VALU counters come from (its own HIP events)
                m = re.search(r'"kernel_ms": ([0-9.]+)', r.stdout.decode(errors="replace"))
                child_ms = float(m.group(1)) if m else None
        res = pmc_summary.summarize(tmp, needle, float(samples_per_launch), passes=tuple(passes), notes=False)
        if not res.get("counters_per_launch", {}).get("FETCH_SIZE"):
            return {"skipped": "the counter passes ran but held no FETCH_SIZE rows for %s" % needle}
        res["child_kernel_ms"] = child_ms
        return res
    except Exception as exc:
        return {"skipped": "counter passes failed: %r" % (exc,)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


# ---- the workload --------------------------------------------------------------------------------------------
def make_signal(synth, signal, period):
    if signal == "fm_tone":
        return synth.fm_tone(period, seed=1234)
    if signal == "white":
        return synth.white_u8(period, seed=1234)
    if signal == "carrier":      # unmodulated, noiseless: every sample hits the same table cell
        return synth.fm_tone(period, seed=1234, deviation=0.0, sigma=0.0)
    if signal == "small":        # weak signal: the table accesses stay within a few cells
        return synth.fm_tone(period, seed=1234, amplitude=6.0, sigma=1.0)
    if signal == "large":        # strong signal: a wide ring through the table
        return synth.fm_tone(period, seed=1234, amplitude=120.0)
    return synth.fm_tone(period, seed=1234, deviation=3000.0)   # "quiet": speech-like deviation


# BASELINE configs[4] ("squelch threshold raised so blocks gate", SURVEY 8(d) Config 5): every channel's row is made of
# loud (carrier amplitude 60) and quiet (amplitude 2) blocks in a pattern that depends on its job-wide index, period 4
# blocks, and the threshold sits at -60 dBFS.  With the Harris AGC running (it raises the IF gain over quiet stretches,
# and the squelch compares level - gain) the steady state is: class 0 (LLLL) always open, class 1 (LQQL) loses one block
# in four, class 2 (QQQL) two, class 3 (LLQQ) one: a quarter of all blocks is rejected, and every channel keeps running -
# the filters see the concatenation of the allowed blocks (IqDataProcessor.cc:793; oracle-checked in tests/test_gpu_scale.py).
GATE_PATTERNS = ((1, 1, 1, 1), (1, 0, 0, 1), (0, 0, 0, 1), (1, 1, 0, 0))
GATE_THRESHOLD_DBFS = -60


def gating_rows(synth, n, block_samples=16384):
    """The four row classes of configs[4] as uint8 arrays of n samples each."""
    loud = synth.fm_tone(n, seed=1234)
    quiet = synth.fm_tone(n, seed=1234, amplitude=2.0, sigma=1.0)
    bb = 2 * block_samples
    rows = []
    for pat in GATE_PATTERNS:
        rows.append(np.concatenate([(loud if pat[b % 4] else quiet)[b * bb:(b + 1) * bb] for b in range(max(1, 2 * n // bb))]))
    return rows


def per_channel_rows(torch, row_u8, n_ch, first_global, row_bytes, chunk=256):
    """[n_ch][row_bytes] uint8 on row_u8's device: channel c (job-wide index g = first_global + c) gets the periodic
    signal row_u8 rolled by 2 * ((g * 37) % 1009) bytes, with four bytes of its own at the front (g, little endian,
    xor-ed in)."""
    dev = row_u8.device
    period = row_u8.numel()
    out = torch.empty((n_ch, row_bytes), dtype=torch.uint8, device=dev)
    t = torch.arange(row_bytes, device=dev, dtype=torch.int64)
    for c0 in range(0, n_ch, chunk):
        g = torch.arange(c0, min(c0 + chunk, n_ch), device=dev, dtype=torch.int64) + first_global
        shift = 2 * ((g * 37) % 1009)
        out[c0:c0 + g.numel()] = row_u8[(t.unsqueeze(0) + shift.unsqueeze(1)) % period]
    g = torch.arange(n_ch, device=dev, dtype=torch.int64) + first_global
    for b in range(4):
        out[:, b] ^= ((g >> (8 * b)) & 0xff).to(torch.uint8)
    return out


def channel_plan(mode, n_ch, first_global):
    """(modes, rotation selectors) of this rank's channels: a function of the channel's index in the whole JOB
    (g = first_global + c), so that the mix is the same however many ranks share it.  The at-size tests run these very
    lists for the offsets ranks 1..7 start at (tests/test_gpu_bench_paths.py)."""
    if mode == "mixed":          # BASELINE configs[3]: channel % 5 -> {AM, FM, WBFM, LSB, USB}
        return [["am", "fm", "wbfm", "lsb", "usb"][(first_global + c) % 5] for c in range(n_ch)], [1] * n_ch
    if mode == "ssb_stress":     # BASELINE configs[4]
        return (["lsb" if (first_global + c) % 2 == 0 else "usb" for c in range(n_ch)],
                [(1, 0, -1)[(first_global + c) % 3] for c in range(n_ch)])
    return [mode] * n_ch, [1] * n_ch


def _set_runs(setter, values):
    c0 = 0
    for c in range(1, len(values) + 1):
        if c == len(values) or values[c] != values[c0]:
            setter(values[c0], first=c0, n=c - c0)
            c0 = c


def configure(eng, mode, n_ch, first_global, squelch):
    """Per-channel settings; `first_global` is this rank's first channel in the whole job."""
    modes, rots = channel_plan(mode, n_ch, first_global)
    _set_runs(eng.set_mode, modes)
    if any(r != 1 for r in rots):
        _set_runs(eng.set_rotation, rots)
    if mode == "ssb_stress":
        eng.agc_set_type(1)      # AGC_TYPE_HARRIS
        eng.agc_enable(True)
        if squelch is None:
            squelch = GATE_THRESHOLD_DBFS
    if squelch is not None:
        eng.set_squelch(squelch)


def gated_rows(torch, loud_u8, quiet_u8, n_ch, first_global, row_bytes, block_bytes=32768):
    """configs[4]'s input: every channel's own roll of the loud and of the quiet signal (per_channel_rows), put together
    block by block after the pattern of the channel's class (g % 4 classes, period 4 blocks)."""
    dev = loud_u8.device
    iq = per_channel_rows(torch, loud_u8, n_ch, first_global, row_bytes)
    lo = per_channel_rows(torch, quiet_u8, n_ch, first_global, row_bytes)
    which = (torch.arange(n_ch, device=dev) + first_global) % len(GATE_PATTERNS)
    pat = torch.tensor(GATE_PATTERNS, dtype=torch.bool, device=dev)           # [class][block % 4]: True = loud
    n_blk = max(1, row_bytes // block_bytes)
    is_loud = pat.index_select(0, which)[:, torch.arange(n_blk, device=dev) % 4]   # [n_ch][n_blk]
    v_iq, v_lo = iq.view(n_ch, n_blk, -1), lo.view(n_ch, n_blk, -1)
    v_iq.copy_(torch.where(is_loud.unsqueeze(-1), v_iq, v_lo))
    return iq


def rank_body(args, rank, world, dev, make_engine, dist, torch, order_streams=None):
    """What one rank does: stage the input, W untimed steps, K timed steps between barriers, the slowest rank's
    clock, and (rank 0) the result.  Engine, device and process group come from the caller, so that the CPU tests
    drive the very same control flow with a stand-in engine over gloo (tests/test_shard_gloo.py)."""
    from rtlsdrdiags_amd import shard, synth

    n = 1 << args.log2_samples
    n_ch = args.channels
    period = min(n, 1 << 24)
    period_u8 = make_signal(synth, args.signal, period)   # the same seeded signal on every rank and channel
    first_global, _ = shard.channel_range(rank, world, n_ch * world)
    gating = args.mode == "ssb_stress" and args.signal == "fm_tone" and n == period
    if gating:   # configs[4]: loud / quiet blocks per channel class, so that the raised squelch really rejects blocks
        loud = torch.from_numpy(synth.fm_tone(n, seed=1234)).to(dev)
        quiet = torch.from_numpy(synth.fm_tone(n, seed=1234, amplitude=2.0, sigma=1.0)).to(dev)
        iq = gated_rows(torch, loud, quiet, n_ch, first_global, 2 * n)
        del loud, quiet
    elif n_ch == 1:
        iq = torch.from_numpy(period_u8).to(dev).repeat(n // period)
    else:
        # Every channel its own data (SURVEY 8(d) Config 3; VERDICT r3: copies of one row make a P wave's lanes gather
        # the same table cells at the same time): the seeded signal rolled by 2 * ((g * 37) % 1009) bytes - whole samples,
        # g the channel's index in the whole job - and four bytes of the channel's own at the front.
        iq = per_channel_rows(torch, torch.from_numpy(period_u8).to(dev), n_ch, first_global, 2 * n)
    n_blocks = max(1, 2 * n // 32768)
    pcm = torch.zeros(n_ch * (n // 32), dtype=torch.int16, device=dev)
    # Two sets of the small per-call outputs, used in turn: under IQD_F_PREPASS_OVERLAP the pre-pass of call N + 1
    # writes pcm_count / magnitude / signal_present while call N's pipelines may still run, so a caller must not hand the
    # call-before's buffers in again (include/iqdemod.h) - as a continuous receiver would not.  The PCM buffer is written by
    # the pipelines, which run in order: one is enough.
    outs = [(torch.zeros(n_ch, dtype=torch.int32, device=dev), torch.zeros(n_ch * n_blocks, dtype=torch.int32, device=dev),
             torch.zeros(n_ch * n_blocks, dtype=torch.uint8, device=dev)) for _ in range(2)]
    step_no = [0]
    cnt, mag, allowed = outs[0]
    sync = (lambda: torch.cuda.synchronize()) if dev.type == "cuda" else (lambda: None)
    sync()

    flags = (1 if args.no_magnitude else 0) | {"tiles": 2, "stream": 4}.get(args.wbfm_path, 0)
    # a squelch that can close: the pre-pass (magnitudes, decisions) of step N + 1 overlaps the pipelines of step N
    # (IQD_F_PREPASS_OVERLAP; the input is resident and complete before any step is queued, which is what the flag asks for)
    prepass_overlap = (args.mode == "ssb_stress" or args.squelch is not None) and not args.inline_prepass
    if prepass_overlap:
        flags |= 8
    eng = make_engine(n_channels=n_ch, flags=flags)
    configure(eng, args.mode, n_ch, first_global, args.squelch)
    gatherer, native_gather = None, False
    if args.gather and dist is not None:
        if dev.type == "cuda" and not args.torch_gather:   # the engine's own RCCL gather (iqd_gather_*), on its stream
            gatherer, native_gather = shard.NativeGatherer(eng, n_ch, n // 32, dev), True
        else:                                              # torch.distributed tensors (the CPU tests run this one over gloo)
            gatherer = shard.PcmGatherer(n_ch, n // 32, dev)

    chunks = max(1, min(getattr(args, "channel_chunks", 1), n_ch))

    def step():
        cnt, mag, allowed = outs[step_no[0] & 1]
        step_no[0] += 1
        if chunks > 1:
            # the call in channel chunks (sub-range accepts, one after the other on the engine's stream): with the overlapped
            # pre-pass, chunk k + 1's magnitudes are taken while chunk k's pipelines run, and a chunk small enough for the
            # Infinity Cache could be read from there the second time (DESIGN.md 4.6 has the measurement)
            for k in range(chunks):
                c0, c1 = n_ch * k // chunks, n_ch * (k + 1) // chunks
                eng.accept_device(iq.data_ptr() + c0 * 2 * n, 2 * n, pcm.data_ptr() + c0 * (n // 32) * 2, cnt.data_ptr() + c0 * 4,
                                  mag.data_ptr() + c0 * n_blocks * 4, allowed.data_ptr() + c0 * n_blocks, first=c0, n=c1 - c0)
        elif args.no_magnitude:
            eng.accept_device(iq.data_ptr(), 2 * n, pcm.data_ptr())
        else:
            eng.accept_device(iq.data_ptr(), 2 * n, pcm.data_ptr(), cnt.data_ptr(), mag.data_ptr(), allowed.data_ptr())
        if gatherer is not None and native_gather:
            gatherer.gather(pcm.view(n_ch, -1), cnt)   # queued on the engine's stream: ordered by construction
        elif gatherer is not None:
            if order_streams is not None:
                order_streams(eng, True)    # the collective's stream waits for the engine's kernels (no host sync)
            else:
                eng.synchronize()
            gatherer.gather(pcm.view(n_ch, -1), cnt)
            if order_streams is not None:
                order_streams(eng, False)   # and the engine's next step waits for the gatherer's copies out of pcm / cnt

    # From idle: what a default-length run measures on a device whose clocks have not settled - the W
    # warm-up steps, then K steps on the host's clock - before the settle phase below.  Reported beside the settled figure
    # (--full only).
    from_idle_ms = None
    if getattr(args, "full", False) and getattr(args, "prewarm_ms", 0.0) > 0 and not getattr(args, "no_from_idle", False):
        eng.synchronize()
        time.sleep(0.25)                                  # (staging the input was load, too: let the device fall idle)
        for _ in range(args.warmup):
            step()
        eng.synchronize()
        if dist is not None:
            dist.barrier()
        t_idle = time.perf_counter()
        for _ in range(args.steps):
            step()
        eng.synchronize()
        from_idle_ms = 1e3 * (time.perf_counter() - t_idle) / args.steps
        if dist is not None:
            dist.barrier()

    # Clock settle: the same step, untimed, for about --prewarm-ms.  A count, not a clock: every rank must run the same
    # number of steps (a gather inside the step is a collective), so it is derived from the workload's size alone.
    prewarm_steps = 0
    if getattr(args, "prewarm_ms", 0.0) > 0:
        est_step_s = max(float(n) * n_ch / 600e9, 20e-6)
        prewarm_steps = int(min(2000, max(1, round(args.prewarm_ms * 1e-3 / est_step_s))))
        for k in range(prewarm_steps):
            step()
            if k % 16 == 15:
                eng.synchronize()       # (bounds the queue; the device stays busy: the host enqueues faster than it drains)
    for _ in range(args.warmup):
        step()
    eng.synchronize()
    sync()
    if dist is not None:
        dist.barrier()
    eng.set_profiling(not getattr(args, "no_kernel_events", False))
    k0 = eng.stats()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    eng.synchronize()
    sync()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    k1 = eng.stats()
    eng.set_profiling(False)
    if rank == 0 and getattr(args, "dump_outputs", None):
        dump_outputs(args.dump_outputs, torch, pcm.view(n_ch, -1), None if args.no_magnitude else outs[(step_no[0] - 1) & 1])
    per_rank_ms, rccl = None, None
    if dist is not None:
        mine = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        per_rank_ms = [round(1e3 * float(t.item()) / args.steps, 4) for t in every]
        elapsed = shard.max_over_ranks(elapsed, dev)
        # what the collective library itself saw (SCALE records: "RCCL saw N ranks")
        rccl = {"backend": dist.get_backend(), "ranks": dist.get_world_size()}
        if native_gather:
            info = gatherer.info()
            rccl.update({"version": info["version"], "ranks": info["ranks"], "communicator": "iqd_gather_* (engine's own, C ABI)",
                         "library_reused": info["library_reused"]})
        elif dev.type == "cuda":
            try:
                rccl["version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception:
                pass

    out = None
    if rank == 0:
        total_samples = float(n) * n_ch * args.steps * world
        launches = max(1, k1["chain_kernel_count"] - k0["chain_kernel_count"])
        kern_ms = (k1["chain_kernel_ms"] - k0["chain_kernel_ms"]) / launches
        streamed = k1.get("stream_launches", 0) - k0.get("stream_launches", 0) > 0
        st_launches = k1.get("stream_launches", 0) - k0.get("stream_launches", 0)
        ch_launches = k1.get("kernel_launches", 0) - k0.get("kernel_launches", 0)
        kernels_ran = ("streaming pipelines" if st_launches == ch_launches and ch_launches else
                       "tile kernels" if st_launches == 0 else
                       "%d of %d chain launches as streaming pipelines, the rest as tile kernels" % (st_launches, ch_launches))
        mixed_one = k1.get("mixed_launches", 0) - k0.get("mixed_launches", 0) > 0
        if mixed_one:
            kernels_ran = "every family's streaming pipeline as a range of one launch's workgroups (mixed_stream_kernel)"
        if args.mode == "mixed":
            # (every launch of the step either way: the one launch + its followers, or - several families as kernels of their own
            #  on side streams - from in front of the fork to behind the join and the closing launch, iqd_engine.cpp)
            timed, timed_samples = ("mixed_stream_kernel (all families' streaming pipelines in one launch) + mixed_tail_kernel" if mixed_one else
                                    "every family's kernels on their side streams, fork to join"), n * n_ch
        elif args.mode in ("am", "lsb", "usb", "ssb_stress"):
            timed, timed_samples = ("d4_stream_kernel" if streamed else "am_chain_kernel") + " + its DC-removal kernels", n * n_ch
            if gating or args.squelch is not None:   # a gated call: the timed kernels see the open blocks only and the magnitude
                timed_samples = None                 # pre-pass is not among them - price the whole step against all its bytes
        elif args.mode == "fm":
            timed, timed_samples = ("d4_stream_kernel" if streamed else "fm_chain_kernel"), n * n_ch
        else:
            timed, timed_samples = ("wbfm_stream_kernel + wbfm_stream_fixup_kernel" if streamed else "wbfm_chain_kernel"), n * n_ch
        if True:   # (the engine's event pair closes behind the step's LAST launch in every arrangement: iqd_engine.cpp, evp_open)
            timed += " + the step's closing launch (repair check, state commit, tails, squelch pass): every launch of the step"
        prof, prof_path = profile_summary(args.tag) if args.tag else (None, None)
        needle = {"wbfm": "wbfm_stream_kernel" if streamed else "wbfm_chain_kernel", "fm": "d4_stream_kernel" if streamed else "fm_chain_kernel",
                  "am": "d4_stream_kernel" if streamed else "am_chain_kernel",
                  "mixed": "mixed_stream_kernel"}.get("am" if args.mode in ("am", "lsb", "usb", "ssb_stress") else args.mode)
        live = None
        if (world == 1 and dev.type == "cuda" and getattr(args, "full", False) and not args.no_live_pmc
                and (timed_samples is not None or mixed_one or args.mode != "mixed")):
            live = live_pmc(args.argv, needle, timed_samples or n * n_ch,   # (counters per launch of the dominant kernel)
                            passes=getattr(args, "pmc_passes", None) or ("fetch", "write", "sq1"))
        roof = {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "kernel": timed, "kernel_ms": round(kern_ms, 4)}
        if timed_samples is not None and kern_ms > 0:
            achieved = ALGO_BYTES_PER_SAMPLE * timed_samples / (kern_ms * 1e-3) / 1e9
            roof.update({"achieved": round(achieved, 1), "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "algorithmic_bytes_per_launch": ALGO_BYTES_PER_SAMPLE * timed_samples})
        else:   # several families side by side: price the whole step against the bytes it moves
            achieved = ALGO_BYTES_PER_SAMPLE * n * n_ch / (elapsed / args.steps) / 1e9
            roof.update({"achieved": round(achieved, 1), "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "algorithmic_bytes_per_launch": ALGO_BYTES_PER_SAMPLE * n * n_ch,
                         "note": "achieved = algorithmic bytes of the step / step time (every kernel of the call: " +
                                 ("the squelch's magnitude pre-pass and decisions, the gated pipeline on the open blocks, its followers)"
                                  if args.mode != "mixed" else "all families' kernels)")})
        live_note = None
        if live is not None and "skipped" in live:   # say why the line has no live counters
            live_note, live = live["skipped"], None
        src = live or prof
        roof["traffic"] = src.get("derived", {}).get("hbm_bytes_per_launch") if src else None
        if src:   # the second ceiling: vector-ALU issue (SQ_ACTIVE_INST_VALU, 4 cycles per wave-instruction, 1024 SIMDs)
            c = src.get("counters_per_launch", {})
            ms = (live.get("child_kernel_ms") or kern_ms) if live else src.get("kernel_ms_avg")   # time and counters of the same run
            ghz = min(c["GRBM_GUI_ACTIVE"] / 8 / (ms * 1e-3) / 1e9, 2.4) if (live and c.get("GRBM_GUI_ACTIVE") and ms) else src.get("clock_ghz", 2.3)
            if c.get("SQ_ACTIVE_INST_VALU") and ms:
                roof["valu_issue_frac"] = round(c["SQ_ACTIVE_INST_VALU"] * 4 / 1024 / (ghz * 1e9) * 1e3 / ms, 3)
                roof["valu_lane_ops_per_sample"] = round(src.get("derived", {}).get("valu_lane_ops_per_sample", 0.0), 1)
            if c.get("SQ_ACTIVE_INST_VALU") and ms and roof.get("achieved"):
                # Which ceiling binds.  The vector ALUs' busy time, spread evenly over the chip's 1024 SIMDs, is
                # the time this instruction stream would take on perfectly levelled, never-idle vector ALUs: the ceiling of
                # the formulation.  The HBM ceiling is `peak`.  The lower one binds; `achieved_over_ceiling` is how close the
                # kernel runs to it.
                # (at the part's 2.4 GHz maximum clock: the counters are per launch of the dominant kernel, the live time covers the
                #  whole step of a short child run, so a clock derived from the two is not to be trusted here - the maximum clock makes
                #  this the most the formulation could reach, i.e. a ceiling)
                busy_ms = c["SQ_ACTIVE_INST_VALU"] * 4 / 1024 / (MAX_CLOCK_GHZ * 1e9) * 1e3
                algo = ALGO_BYTES_PER_SAMPLE * (timed_samples or n * n_ch)
                ceil_gbs = algo / (busy_ms * 1e-3) / 1e9
                roof["ceilings"] = {"hbm": {"GB/s": HBM_PEAK_GBS, "frac_of_hbm_peak": 1.0},
                                    "valu_issue": {"GB/s": round(ceil_gbs, 1), "frac_of_hbm_peak": round(ceil_gbs / HBM_PEAK_GBS, 4),
                                                   "valu_busy_ms_levelled": round(busy_ms, 4), "clock_ghz": MAX_CLOCK_GHZ,
                                                   "how": "SQ_ACTIVE_INST_VALU x 4 cycles / 1024 SIMDs / 2.4 GHz (the maximum clock): the instruction "
                                                          "stream's time on perfectly levelled, never-idle vector ALUs"}}
                roof["binds"] = "valu_issue" if ceil_gbs < HBM_PEAK_GBS else "hbm"
                roof["achieved_over_binding_ceiling"] = round(roof["achieved"] / min(ceil_gbs, HBM_PEAK_GBS), 3)
            roof["traffic_over_algorithmic"] = round(roof["traffic"] / (ALGO_BYTES_PER_SAMPLE * (timed_samples or n * n_ch)), 3) if roof["traffic"] else None
            roof["counters"] = ("collected in this run: rocprofv3 --pmc passes of the same command (FETCH_SIZE x 2 + WRITE_SIZE per the "
                                "guide's gfx950 correction; per launch of %s)" % needle) if live else prof_path
        elif prof_path:
            roof["counters"] = prof_path   # (says why the committed summary was not used)
        if live_note:
            roof["counters_note"] = "no live counters: " + live_note
        out = {
            "metric": METRIC if args.mode == "wbfm" else METRIC.replace("WBFM chain", "%s chains" % args.mode.upper()),
            "value": round(total_samples / elapsed / 1e6, 1), "unit": "MSamples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 4),
            "from_idle_ms_per_step": None if from_idle_ms is None else round(from_idle_ms, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "int8/int16 Q15 + f32", "data": "synthetic" if args.signal == "fm_tone" else "synthetic (%s)" % args.signal,
            "config": {"workload": args.what or "%s, %d channel(s) per GPU, 2^%d IQ samples per channel per step, uint8 I/Q "
                                                "resident in HBM (not a BASELINE configuration)"
                                                % (args.mode.upper(), n_ch, args.log2_samples),
                       "channels_per_gpu": n_ch, "log2_samples_per_channel": args.log2_samples, "kernels": kernels_ran,
                       "prewarm": "%d untimed steps of the same workload (about %g ms of load) before the %d warm-up steps: clock settle"
                                  % (prewarm_steps, getattr(args, "prewarm_ms", 0.0), args.warmup),
                       "sharding": "independent channels, contiguous range per rank, no data-path collective"
                                   + ("; PCM gathered to rank 0 over RCCL (%s)" % ("iqd_gather_pcm, C ABI" if native_gather else "torch.distributed")
                                      if args.gather else "")},
            "roofline": roof,
            "state_checks": k1["state_checks"] - k0["state_checks"],
            "state_repairs": k1["state_repairs"] - k0["state_repairs"],
            "segment_repairs": k1["segment_repairs"] - k0["segment_repairs"],
        }
        if per_rank_ms is not None:
            out["per_rank_ms"] = per_rank_ms   # every rank's own clock over the K steps (value uses the slowest)
            out["rccl"] = rccl
        if not args.no_magnitude:   # what the squelch did in the last step (rank 0's channels)
            if gating or args.squelch is not None:
                out["config"]["prepass"] = ("one step ahead on its own stream (IQD_F_PREPASS_OVERLAP: magnitudes and decisions of step N + 1 "
                                            "overlap the pipelines of step N)" if prepass_overlap else "inline (each step: pre-pass, then pipelines)")
            cnt, mag, allowed = outs[(step_no[0] - 1) & 1]     # (the last step's)
            open_frac = float(allowed.float().mean().item())
            out["config"]["squelch"] = {"threshold_dbfs": GATE_THRESHOLD_DBFS if (args.squelch is None and args.mode == "ssb_stress") else args.squelch,
                                        "blocks_rejected_frac": round(1.0 - open_frac, 4),
                                        "pcm_samples_per_channel_mean": round(float(cnt.float().mean().item()), 1)}
        if world == 1 and getattr(args, "full", False) and not args.no_host_path and dev.type == "cuda":
            out["host_path"] = host_path(eng, iq, n, n_ch)
        if world == 1 and getattr(args, "full", False) and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(period_u8, args.mode, all_cores=not args.cpu_one_core_only)
    eng.close()
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 20; configs[0]: 61)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed warm-up steps (default 3)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: the from-idle figure, the CPU baseline, the host path, "
                         "the rocprofv3 counter passes, the other configurations (`other_configs`) and configs[0]'s CPU parity check")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the last step's outputs (PCM, counts, magnitudes, squelch flags) as "
                         "DIR/<name>.npy in float32 / float64; a PCM larger than 2^23 samples is written as a fixed, seeded sample of 2^22")
    ap.add_argument("--prewarm-ms", type=float, default=100.0,
                    help="untimed load before the warm-up steps, so that the device's clocks have settled when the timed steps "
                         "start (DESIGN.md section 6: the step time falls by a tenth over the first 25 ms of load); 0 = none")
    ap.add_argument("--no-from-idle", action="store_true", help="skip the from-idle figure (W + K steps before the clock-settle phase)")
    ap.add_argument("--config", type=int, default=None, choices=sorted(CONFIGS), help="BASELINE.json configs[N] preset (default 1)")
    ap.add_argument("--log2-samples", type=int, default=None, help="IQ samples per channel per step (overrides the preset)")
    ap.add_argument("--channels", type=int, default=None, help="channels per GPU (overrides the preset)")
    ap.add_argument("--mode", default=None, help="am|fm|wbfm|lsb|usb|mixed|ssb_stress (overrides the preset)")
    ap.add_argument("--signal", default="fm_tone", choices=["fm_tone", "white", "carrier", "quiet", "small", "large"],
                    help="synthetic input: the FM test tone of SURVEY 8(d) (default) or uniform random bytes, ...")
    ap.add_argument("--no-magnitude", action="store_true", help="IQD_F_NO_MAGNITUDE: skip the per-block squelch magnitudes")
    ap.add_argument("--squelch", type=int, default=None, help="squelch threshold in dBFS (default: the reference's -200, never closes)")
    ap.add_argument("--wbfm-path", default="auto", choices=["auto", "tiles", "stream"], help="pin the WBFM kernel (A/B)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-one-core-only", action="store_true", help="skip the all-host-cores CPU baseline")
    ap.add_argument("--no-host-path", action="store_true", help="skip the PCIe-inclusive iqd_accept_iq measurement")
    ap.add_argument("--gather", action="store_true", help="also gather the PCM to rank 0 over RCCL each step")
    ap.add_argument("--torch-gather", action="store_true", help="with --gather: torch.distributed tensors instead of the engine's own iqd_gather_pcm")
    ap.add_argument("--no-live-pmc", action="store_true", help="do not collect HBM / VALU counters with rocprofv3 child runs")
    ap.add_argument("--channel-chunks", type=int, default=1, help="measurement: each step as this many sub-range calls (channel chunks)")
    ap.add_argument("--inline-prepass", action="store_true",
                    help="squelch-gated runs: the magnitude pre-pass inside each step's own stream order (default: one step ahead, IQD_F_PREPASS_OVERLAP)")
    ap.add_argument("--no-kernel-events", action="store_true",
                    help="diagnostic: time the steps without the engine's per-kernel HIP events (no roofline.kernel_ms then)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="with --full, the default workload (configs[1]) also times configs[0], [2], [3], [4] and AM / USB at 4096 x 2^16 for a "
                         "few steps each and reports them as `other_configs`; this flag skips that")
    ap.add_argument("--pmc-passes", default=None, help=argparse.SUPPRESS)   # fetch,write[,sq1]: which counter passes live_pmc runs (the sub-lines: two)
    ap.add_argument("--force-launch", action="store_true",
                    help="start the ranks through bench.py's own launcher (torch.distributed.run as a child process) even for --gpus 1: "
                         "the N > 1 code path - nccl process group, device_id, the engine's RCCL gatherer - on a one-GPU box")
    ap.add_argument("--standin", default=None, help=argparse.SUPPRESS)   # module:Class of a host-memory engine (CPU tests of the launcher)
    args = ap.parse_args(argv)
    args.argv = list(sys.argv[1:] if argv is None else argv)
    if args.pmc_passes:          # (not handed on to the counter passes' own child runs)
        args.pmc_passes = tuple(x for x in args.pmc_passes.split(",") if x)
        i = args.argv.index("--pmc-passes")
        del args.argv[i:i + 2]
    # (nor the dump: a counter pass must not overwrite the outputs of the run that started it)
    args.argv = [a for i, a in enumerate(args.argv) if not a.startswith("--dump-outputs")
                 and not (i > 0 and args.argv[i - 1] == "--dump-outputs")]
    preset = CONFIGS[1 if args.config is None else args.config]
    if args.warmup is None:
        args.warmup = 3
    if args.steps is None:                       # configs[0]: 64 blocks = 2^20 samples, SURVEY 8(d) Config 1
        args.steps = 61 if (args.config == 0 and args.warmup == 3) else 20
    custom = args.mode is not None or args.channels is not None or args.log2_samples is not None
    args.mode = args.mode or preset["mode"]
    args.channels = args.channels or preset["channels"]
    args.log2_samples = args.log2_samples or preset["log2"]
    same = (args.mode, args.channels, args.log2_samples) == (preset["mode"], preset["channels"], preset["log2"])
    args.what = preset["what"] if (same or not custom) else None
    args.tag = preset["tag"] if (same or not custom) and args.signal == "fm_tone" and not args.no_magnitude else None
    # the driver's own run (`python bench.py --gpus 1 --steps K --warmup W`): configs[1] as the contract names it, nothing pinned
    args.is_default_workload = (args.config in (None, 1) and not custom and args.signal == "fm_tone" and not args.no_magnitude
                                and args.squelch is None and args.wbfm_path == "auto" and not args.gather and args.channel_chunks == 1)
    return args


def self_launch(argv, n_gpus):
    """`python bench.py --gpus N` outside a launcher: start the ranks as a CHILD process (never exec: a process that
    has touched the GPU must not be replaced, and this one must stay to relay the result), one rank per GPU, and pass
    on rank 0's line and the exit code."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n_gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    p = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
    line = None
    for ln in p.stdout.decode(errors="replace").splitlines():
        if ln.startswith('{"metric"'):
            line = ln
        else:
            print(ln, file=sys.stderr)
    if line is not None:
        print(line)
    sys.stdout.flush()
    return p.returncode if (p.returncode != 0 or line is not None) else 1


# What the default workload's --full run times besides its headline: every other BASELINE configuration and the two
# single-family AM / SSB workloads DESIGN.md quotes, each as a child process with a run's own settings.
OTHER_CONFIGS = (["--config", "0"], ["--config", "2"], ["--config", "3"], ["--config", "4"],
                 ["--mode", "am", "--channels", "4096", "--log2-samples", "16"],
                 ["--mode", "usb", "--channels", "4096", "--log2-samples", "16"])
SUB_KEYS = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "config", "roofline", "state_repairs", "block_latency_us",
            "device_ops_per_block", "real_time_factor", "parity")


def other_configs(args):
    """Sub-lines of the default workload's --full run: each one is what `python bench.py <argv> --full` prints, cut down to SUB_KEYS - a CHILD process per
    configuration (the same rank_body, the engine's event timing, HBM traffic from two rocprofv3 --pmc passes of that very command:
    FETCH_SIZE, WRITE_SIZE), so that whatever happens in one of them costs a sub-line and never the headline."""
    import subprocess
    lines = []
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    for argv in OTHER_CONFIGS:
        t0 = time.perf_counter()
        cmd = [sys.executable, os.path.abspath(__file__)] + argv + ["--full", "--no-other-configs", "--no-host-path", "--no-from-idle",
                                                                    "--pmc-passes", "fetch,write"]
        if argv != ["--config", "0"]:   # (configs[0]: its 64 blocks, with the CPU chain beside them - the parity check of that file)
            cmd += ["--steps", "20", "--warmup", "3", "--prewarm-ms", "100", "--no-cpu-baseline"]   # (the settings of a run of its own)
        if args.no_live_pmc:
            cmd += ["--no-live-pmc"]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT, timeout=420)
            out = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith('{"metric"')]
            if r.returncode != 0 or not out:
                raise RuntimeError("exit code %d: %s" % (r.returncode, r.stderr.decode(errors="replace")[-300:]))
            d = json.loads(out[-1])
            line = {"argv": " ".join(argv)}
            line.update({k: d[k] for k in SUB_KEYS if k in d})
            line["seconds"] = round(time.perf_counter() - t0, 1)
        except Exception as exc:          # a sub-line must never cost the run its headline
            line = {"argv": " ".join(argv), "error": repr(exc)[:400]}
        lines.append(line)
    return lines


def config0(args):
    """BASELINE configs[0]: one FM channel from a FILE through the C++ IqDataProcessor::acceptIqData in 32768-byte
    blocks (rtlsdrdiags_amd/bin/iqdemod_file: the reference's radioApp.cc / demod.cc shape), one block per call - the
    reference's real operating point (DataConsumer.cc:333-346).  A step is one block; the first `warmup` blocks of the
    file are not timed.  With --full the PCM is held to the CPU chain's, which is timed beside it on the same file."""
    import subprocess
    import tempfile
    from rtlsdrdiags_amd import synth
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_file")
    n_blocks = args.warmup + args.steps
    u8 = synth.fm_tone(n_blocks * 16384, seed=1)
    with tempfile.TemporaryDirectory() as tmp:
        src, timing = os.path.join(tmp, "fm_u8.iq"), os.path.join(tmp, "timing.txt")
        u8.tofile(src)
        with open(src, "rb") as fin:
            r = subprocess.run([tool, "2", "timing=" + timing], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0:
            sys.exit("iqdemod_file failed (%d): %s" % (r.returncode, r.stderr.decode(errors="replace")))
        pcm = np.frombuffer(r.stdout, dtype=np.int16)
        with open(timing) as f:
            head = f.readline().split()
            us = np.array([float(x) for x in f.read().split()])
    counts = dict(zip(head[0::2], map(int, head[1::2])))
    t = us[args.warmup:]
    out = {
        "metric": METRIC.replace("WBFM chain", "FM chain (file source, one block per call)"),
        "value": round(16384 * len(t) / t.sum(), 3), "unit": "MSamples/s", "n_gpus": 1, "steps": int(len(t)), "warmup": args.warmup,
        "ms_per_step": round(float(t.mean()) / 1e3, 5), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "int8/int16 Q15 + f32", "data": "synthetic",
        "config": {"workload": args.what, "channels_per_gpu": 1, "block_bytes": 32768,
                   "host_path": "file -> fread -> IqDataProcessor::acceptIqData (C++) -> iqd_accept_iq (upload, kernels, PCM download) "
                                "-> PCM callback -> fwrite; PCIe-inclusive by nature"},
        "block_latency_us": {"p50": round(float(np.percentile(t, 50)), 1), "p99": round(float(np.percentile(t, 99)), 1),
                             "max": round(float(t.max()), 1), "first_block": round(float(us[0]), 1)},
        "device_ops_per_block": {"kernel_launch_calls": round(counts["launches"] / counts["blocks"], 2),
                                 "copies_and_fills": round(counts["copies"] / counts["blocks"], 2)},
        "real_time_factor": round(16384 * len(t) / t.sum() / 0.256, 1),
        "roofline": {"bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s", "achieved": round(2.0625 * 16384 * len(t) / t.sum() / 1e3, 3),
                     "frac": round(2.0625 * 16384 * len(t) / t.sum() / 1e3 / HBM_PEAK_GBS, 6), "traffic": None,
                     "note": "one 32 KiB block per call: latency-bound by construction (a 64 ms block every 64 ms is the "
                             "reference's operating point); the throughput roofline is configs[1]'s business"},
    }
    if args.dump_outputs:          # (the PCM of the whole file: the last step's block is its tail)
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "pcm.npy"), pcm.astype(np.float32))
    if args.full and not args.no_cpu_baseline:
        chain, kind = _cpu_chain("fm")
        t0 = time.perf_counter()
        ref, _, _ = chain.accept_stream(u8)
        dt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(len(u8) / 2 / dt / 1e6, 3), "unit": "MSamples/s", "cores": 1, "kind": kind,
                               "us_per_block": round(1e6 * dt / n_blocks, 1),
                               "sample": "the same %d blocks through IqDataProcessor::acceptIqData on one host core" % n_blocks}
        out["parity"] = "PCM identical to the CPU chain" if np.array_equal(pcm, ref) else "PCM DIFFERS from the CPU chain"
        if not np.array_equal(pcm, ref):
            print(json.dumps(out))
            sys.exit("bench.py --config 0: PCM differs from the CPU chain")
    return out


def main():
    args = parse_args()
    if args.config == 0:
        print(json.dumps(config0(args)))
        return
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is None and (args.gpus > 1 or args.force_launch):
        if not args.standin:   # before any rank starts (counting devices does not initialise the GPU on this image)
            import torch
            visible = torch.cuda.device_count()
            if args.gpus > visible:
                sys.exit("bench.py: --gpus %d but this host shows %d GPU(s); nothing was started" % (args.gpus, visible))
        sys.exit(self_launch(sys.argv[1:], args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(world_env or "1")
    args.gpus = world

    import torch
    if args.standin:
        # CPU test of the launcher and the rank body (tests/test_shard_gloo.py): a stand-in engine over host memory,
        # gloo instead of RCCL.  The line says so in `data`; nothing here measures the product.
        import importlib
        import torch.distributed as dist
        mod, cls = args.standin.split(":")
        factory = getattr(importlib.import_module(mod), cls)
        dist.init_process_group("gloo")
        out = rank_body(args, rank, world, torch.device("cpu"), lambda n_channels, flags: factory(n_channels, flags, rank), dist, torch)
        if out is not None:
            out["data"] = "STAND-IN ENGINE on the CPU (launcher test, not a measurement)"
            print(json.dumps(out))
        dist.barrier()
        dist.destroy_process_group()
        return
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (the engine has no CPU path)")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1 or "TORCHELASTIC_RUN_ID" in os.environ:   # launched by torch.distributed.run (also with 1 rank)
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from rtlsdrdiags_amd import capi

    def make_engine(n_channels, flags):
        return capi.Engine(n_channels=n_channels, device=local_rank, flags=flags)

    def order_streams(eng, engine_first):
        """engine_first: torch's current stream (where the gatherer's copies and the collective are enqueued) waits
        for the engine's stream; else the engine's stream waits for torch's (the next step must not overwrite pcm / cnt
        while the gatherer is still copying out of them: ADVICE r2)."""
        ext = torch.cuda.ExternalStream(eng.stream_handle())
        if engine_first:
            torch.cuda.current_stream().wait_stream(ext)
        else:
            ext.wait_stream(torch.cuda.current_stream())

    out = rank_body(args, rank, world, torch.device("cuda", local_rank), make_engine, dist, torch, order_streams)
    # (--full on the default workload only: a run trimmed with --no-cpu-baseline / --no-host-path is a measurement tool's)
    if (out is not None and world == 1 and dist is None and args.is_default_workload and args.full
            and not (args.no_other_configs or args.no_cpu_baseline or args.no_host_path)):
        out["other_configs"] = other_configs(args)
    if out is not None:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
