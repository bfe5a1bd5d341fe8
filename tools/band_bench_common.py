"""What tools/spectrum_bench.py, detect_bench.py, track_bench.py, measure_bench.py and tracklog_bench.py share: the command
line, the standing capture, the chain Spectrum -> Detector -> Tracker -> Measure -> TrackLog set up on device arrays up to the
stage a tool times, the three-round alternation over its calls, and the print-and-write tail.  Each tool's docstring says what
it measures; the method is the same in all: tools/chan_bench.py's timed() - a host clock around the call and iqd_synchronize,
the median of --steps calls after about --settle-ms of the same call untimed."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STATIONS = [{"offset": -700e3, "kind": "fm", "amplitude": 25.0, "tone": 1000.0},
            {"offset": 250e3, "kind": "am", "amplitude": 25.0, "tone": 700.0}]
N_SRC, BPS, N_BLOCKS, K = 16, 1 << 20, 64, 16         # sources, bytes per source, blocks per source, detection records per row
N_ROWS = N_SRC * N_BLOCKS
STAGES = ("spectrum", "detect", "track", "measure", "tracklog")


def arguments(sizes=True):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--settle-ms", type=float, default=300.0)
    if sizes:
        ap.add_argument("--sizes", default="256,1024,2048")
    ap.add_argument("--no-write", action="store_true", help="print only")
    args = ap.parse_args()
    if sizes:
        args.sizes = [int(v) for v in args.sizes.split(",")]
    return args


def capture(eng):
    """the standing capture on the device: synth.wideband's two stations over noise, one source's 2^19 samples for all 16"""
    from rtlsdrdiags_amd import synth
    d_in = eng.dev_alloc(N_SRC * BPS)
    eng.dev_upload(d_in, np.tile(synth.wideband(BPS // 2, 2048000.0, STATIONS, seed=7), N_SRC))
    return d_in


class Chain:
    """The chain's objects and device arrays at N bins up to `stage` (README's parameters, 8 and 64 slots), with every stage
    before it run so that the stage's inputs stand: the trackers twice - from the second call on every block has its active
    tracks.  max_det sizes the detection array (a tool's busier detector writes into the same one)."""

    def __init__(self, capi, eng, d_in, N, stage, max_det=K):
        self.eng, self.d_in, self.N, self.F = eng, d_in, N, BPS // N_BLOCKS // (2 * N)
        self.objects, self.arrays = [], []
        upto = STAGES.index(stage)
        self.s = self._made(capi.Spectrum(eng, N, n_sources=N_SRC))
        self.d_pow = self._dev(N_ROWS * N * 4)
        if upto >= 1:
            self.det = self._made(capi.Detector(eng, N, max_detections=K))
            self.d_rows, self.d_det = self._dev(N_ROWS * 16), self._dev(N_ROWS * max_det * 32)
            self.spectrum()
        if upto >= 2:
            self.t = {S: self._made(capi.Tracker(eng, N, n_sources=N_SRC, max_detections=K, n_slots=S)) for S in (8, 64)}
            self.d_slots, self.d_blocks = {S: self._dev(N_ROWS * S * 32) for S in (8, 64)}, self._dev(N_ROWS * 16)
            self.detect()
        if upto >= 3:
            self.m = {S: self._made(capi.Measure(eng, N, n_sources=N_SRC, n_slots=S)) for S in (8, 64)}
            self.d_meas = {S: self._dev(N_ROWS * S * 32) for S in (8, 64)}
            for S in (8, 64):
                self.track(S)
                self.track(S)
        if upto >= 4:
            self.max_events = capi.tracklog_defaults()["max_events"]
            self.lg = {S: self._made(capi.TrackLog(eng, n_sources=N_SRC, n_slots=S)) for S in (8, 64)}
            self.d_summary, self.d_events, self.d_counts = self._dev(N_ROWS * 64 * 64), self._dev(N_SRC * self.max_events * 64), self._dev(N_SRC * 16)
            for S in (8, 64):
                self.measure(S)
        eng.synchronize()

    def _made(self, obj):
        self.objects.append(obj)
        return obj

    def _dev(self, nbytes):
        self.arrays.append(self.eng.dev_alloc(nbytes))
        return self.arrays[-1]

    # the calls a tool times; fewer blocks (rows) read the same arrays' first rows, whatever source they belong to
    def spectrum(self):
        self.s.run_device(self.d_in, BPS, self.F, self.d_pow)

    def detect(self, n_rows=N_ROWS, detector=None):
        (detector or self.det).run_device(self.d_pow, n_rows, self.d_rows, self.d_det)

    def track(self, S, n_blocks=N_BLOCKS):
        self.t[S].run_device(self.d_rows, self.d_det, n_blocks, self.d_slots[S], self.d_blocks)

    def measure(self, S, n_blocks=N_BLOCKS):
        self.m[S].run_device(self.d_pow, self.d_rows, self.d_slots[S], n_blocks, self.d_meas[S])

    def log(self, S, n_blocks=N_BLOCKS):
        self.lg[S].run_device(self.d_slots[S], self.d_meas[S], n_blocks, self.d_summary, self.d_events, self.d_counts)

    def download(self, ptr, nbytes, dtype):
        return self.eng.dev_download(ptr, nbytes).view(dtype)

    def close(self):
        for o in reversed(self.objects):
            o.close()
        for p in self.arrays:
            self.eng.dev_free(p)


def fm_accept_rig(n_ch=4096, nbytes=131072, n_pcm=2048):
    """What tools/tones_bench.py and fsk_bench.py stand on: (eng, d_iq, d_pcm, d_cnt, accept) - an FM engine of n_ch channels, a
    tone's capture for each on the device, and accept(), the call that leaves n_pcm samples per channel in d_pcm and the counts
    in d_cnt (run once here, and checked)"""
    from rtlsdrdiags_amd import capi, synth
    eng = capi.Engine(n_ch)
    eng.set_mode("fm")
    d_iq, d_pcm, d_cnt = eng.dev_alloc(n_ch * nbytes), eng.dev_alloc(n_ch * n_pcm * 2), eng.dev_alloc(n_ch * 4)
    eng.dev_upload(d_iq, synth.fm_tone(nbytes // 2, seed=3, deviation=2500.0))
    eng.dev_tile(d_iq, nbytes, n_ch * nbytes)

    def accept():
        eng.accept_device(d_iq, nbytes, d_pcm, d_cnt)

    accept()
    eng.synchronize()
    assert (eng.dev_download(d_cnt, n_ch * 4, np.uint32) == n_pcm).all()
    return eng, d_iq, d_pcm, d_cnt, accept


def alternate(calls, eng, args, after=None):
    """The calls one after the other, three times over -> ({key: [each round's median ms]}, {key: the median of those});
    after(key) runs behind a call's timing."""
    from chan_bench import timed
    ms = {k: [] for k in calls}
    for _ in range(3):
        for k, fn in calls.items():
            ms[k].append(round(timed(fn, eng.synchronize, args.steps, args.settle_ms)[0], 4))
            if after:
                after(k)
    return ms, {k: float(np.median(v)) for k, v in ms.items()}


def finish(line, args, name):
    """prints the line; writes it to profiles/<name> unless --no-write"""
    print(json.dumps(line))
    if not args.no_write:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", name), "w") as f:
            f.write(json.dumps(line) + "\n")
