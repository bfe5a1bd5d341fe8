"""Diagnostic: randomized band-chain runs on an MI355X, every array bit for bit against the models written from the header
(include/iqdemod.h: "Band spectrum", "Band activity", "Band tracks"; tests/spectrum_model.py, tests/detect_model.py,
tests/track_model.py).

    python tools/band_fuzz.py --kind spectrum|detect|track|chain [--seed S] [--cases C]     a campaign
    python tools/band_fuzz.py --kind detect --seed S --case I                                one case again

Case I of seed S is drawn from numpy's default_rng([S, I]) and from nothing else, so (seed, index) names a case on every
machine.  Every case is drawn without a GPU (draw_spectrum, draw_detect, draw_track, draw_chain) and then run
(run_*); the case functions take gpu=False, which draws the case and runs the model alone, so that the CPU tier
(tests/test_band_fuzz_host.py) holds the very cases of SLICES - the slices of tests/test_gpu_band_fuzz.py - to the models'
defects and to a list of structural conditions before they go to the GPU.

The draws are structured: about every second parameter comes from a list of edges, the rest at random, all inside the
ranges the header documents (the models' check_cfg / check_window assert them).  Refusals are not fuzzed.

  spectrum  N, format, window (default, random, negative entries, on the 256 sum |w| limit), F around the kernel's frame
            tiles (16, 32, 48, 64 and one either side), sources, blocks, bytes (white, rails, constants, small, mixed)
  detect    rows of floor noise (zeros, one value, values that differ in one byte, near 2^32, sparse, uniform) with planted
            runs: lengths around min_width and around 64, gaps of g, g + 1, g + 2, starts and ends at 62 .. 65 modulo 64,
            holes of up to g bins (some over a multiple of 64), equal peaks, 2^32 - 1, a run over the guard
  track     a script of stations that are born, drift, fade and return, drawn block by block against the model's own
            slots, so that detections can be put at exactly G and G + 1 from a track and half way between two tracks;
            n_found above K; garbage past D; split calls, a reset, get_state after the last call
  chain     keyed carriers in noise per source; Spectrum, Detector and Tracker queued in device form on one stream with one
            synchronise at the end, in one call or two, in device buffers that are reused from case to case uncleared"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                     # noqa: E402
from rtlsdrdiags_amd import capi, synth                # noqa: E402
from tests import detect_model as dm                   # noqa: E402
from tests import spectrum_model as sm                 # noqa: E402
from tests import track_model as tm                    # noqa: E402

N_SET = sm.N_SET
M32 = 2 ** 32 - 1
BOUND_SUM = (2 ** 31 - 256) // 256
F_EDGES = (1, 2, 15, 16, 17, 31, 32, 33, 40, 47, 48, 49, 63, 64, 65, 80, 112, 128, 130)
ROW_EDGES = (1, 2, 3, 4, 5, 7, 8, 9)
RATE = 2048000.0
SPECTRUM_BUDGET = 2 ** 27      # N^2 x frames of a case: what the spectrum model's matrix products may cost
TRACK_BUDGET = 120000          # sources x blocks x slots x detections of a case: the tracker model's inner loop
# (seed, cases): tests/test_gpu_band_fuzz.py's, held to the proof by tests/test_band_fuzz_host.py
SLICES = {"spectrum": (9301, 60), "detect": (9302, 150), "track": (9303, 90), "chain": (9304, 16)}


def case_rng(seed, index):
    return np.random.default_rng([int(seed), int(index)])


def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def edge_or(rng, edges, lo, hi, log=False):
    """about every second draw from the edges (those inside lo .. hi), else lo .. hi uniformly, or uniformly in the logarithm"""
    edges = [e for e in edges if lo <= e <= hi]
    if edges and rng.random() < 0.5:
        return int(pick(rng, edges))
    if log:
        return int(min(hi, max(lo, round(2.0 ** rng.uniform(np.log2(max(lo, 1)), np.log2(hi))))))
    return int(rng.integers(lo, hi + 1))


class Context:
    """What every case shares: the phasor table and, with a GPU, one engine and the chain cases' device buffers."""

    def __init__(self, gpu=True):
        self.capi, self.P, self.gpu = capi, capi.channelizer_phasor_table(), gpu
        self.eng = capi.Engine(1) if gpu else None
        self.stats, self.pool = {}, {}

    def count(self, key, n=1):
        self.stats[key] = self.stats.get(key, 0) + int(n)

    def buffer(self, name, n_bytes):
        """a device buffer of at least n_bytes that keeps what the last case left in it"""
        ptr, size = self.pool.get(name, (0, 0))
        if size < n_bytes:
            if ptr:
                self.eng.dev_free(ptr)
            size = max(n_bytes, 2 * size)
            ptr = self.eng.dev_alloc(size)
            self.eng.dev_upload(ptr, np.full(size, dm.STALE, np.uint8))
            self.pool[name] = (ptr, size)
        return ptr

    def close(self):
        if self.eng is not None:
            for ptr, _ in self.pool.values():
                self.eng.dev_free(ptr)
            self.pool = {}
            self.eng.close()
            self.eng = None


def differs(what, got, want):
    """None, or where two arrays first differ"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return "%s: shape / dtype %s %s, model %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.tobytes() == want.tobytes():
        return None
    bad = np.argwhere(got != want)
    at = tuple(bad[0])
    return "%s differs in %d entries, first at %s: got %s, model %s" % (what, len(bad), at, got[at], want[at])


# ---------------------------------------------------------------------------------------------------- spectrum

def draw_window(rng, N):
    """(kind, window argument): None -> the default window"""
    r = rng.random()
    if r < 0.35:
        return "default", None
    smax = min(32639, BOUND_SUM // N)
    if r < 0.5:                                            # on the limits: every entry as large as the sum allows
        sign = rng.choice([-1, 1], N) if rng.random() < 0.5 else np.ones(N, np.int64)
        w = np.full(N, smax, np.int64)
        if smax < 32639:
            w[:min(N, BOUND_SUM - N * smax)] += 1
        return "limit", (w * sign).astype(np.int16)
    s = int(2.0 ** rng.uniform(3, np.log2(smax)))
    if rng.random() < 0.6:
        return "signed %d" % s, rng.integers(-s, s + 1, N).astype(np.int16)
    return "positive %d" % s, rng.integers(0, s + 1, N).astype(np.int16)


def draw_bytes(rng, n_src, n_frames, N):
    """(kind, [n_src, 2 N n_frames] uint8): the capture's bytes, whatever the format reads them as"""
    kind = pick(rng, ("white", "white", "rails", "const", "low", "mixed", "mixed"))
    shape = (n_src, n_frames, 2 * N)
    if kind == "white":
        b = rng.integers(0, 256, shape, dtype=np.uint8)
    elif kind == "rails":
        b = rng.choice(np.array([0, 255, 127, 128], np.uint8), shape)
    elif kind == "const":                                  # one pair all along, every second time on the rails
        pair = rng.integers(0, 256, 2, dtype=np.uint8) if rng.random() < 0.5 else rng.choice(np.array([0, 255, 127, 128], np.uint8), 2)
        b = np.broadcast_to(np.tile(pair, N), shape).copy()
    elif kind == "low":
        amp = int(2.0 ** rng.uniform(0, 5))
        b = (int(pick(rng, (0, 128))) + rng.integers(-amp, amp + 1, shape)).astype(np.uint8)
    else:                                                  # white, with frames of rails and constants among it
        b = rng.integers(0, 256, shape, dtype=np.uint8)
        for j in range(n_src):
            for f in np.flatnonzero(rng.random(n_frames) < 0.4):
                if rng.random() < 0.5:
                    b[j, f] = rng.choice(np.array([0, 255, 127, 128], np.uint8), 2 * N)
                else:
                    b[j, f] = np.tile(rng.integers(0, 256, 2, dtype=np.uint8), N)
    return kind, np.ascontiguousarray(b.reshape(n_src, -1))


def draw_spectrum(rng):
    N = int(pick(rng, N_SET))
    fmt = pick(rng, ("u8", "s8"))
    wkind, window = draw_window(rng, N)
    F = int(pick(rng, F_EDGES)) if rng.random() < 0.5 else int(rng.integers(1, 131))
    n_src, blocks = int(rng.integers(1, 4)), int(rng.integers(1, 5))
    while N * N * F * n_src * blocks > SPECTRUM_BUDGET:     # large N takes fewer frames
        r = rng.random()
        if r < 0.4 and blocks > 1:
            blocks -= 1
        elif r < 0.6 and n_src > 1:
            n_src -= 1
        else:
            smaller = [e for e in F_EDGES if e < F]
            F = int(pick(rng, smaller)) if smaller and rng.random() < 0.7 else max(1, F // 2)
    ikind, b = draw_bytes(rng, n_src, F * blocks, N)
    if ikind == "const" and rng.random() < 0.5:             # with the largest window of one sign: block sums past 2^32
        smax = min(32639, BOUND_SUM // N)
        window = np.full(N, smax, np.int16)
        window[:min(N, BOUND_SUM - N * smax) if smax < 32639 else 0] += 1
        wkind = "limit"
    wide = b if fmt == "u8" else b.view(np.int8)
    return dict(N=N, fmt=fmt, wkind=wkind, window=window, F=F, n_src=n_src, blocks=blocks, ikind=ikind, wide=wide,
                fill=int(rng.integers(0, 256)))


def describe_spectrum(c):
    return "N %d %s window %s F %d sources %d blocks %d input %s fill 0x%02x" % (
        c["N"], c["fmt"], c["wkind"], c["F"], c["n_src"], c["blocks"], c["ikind"], c["fill"])


def spectrum_model(c, P):
    w = sm.default_window(c["N"], P)[0] if c["window"] is None else c["window"]
    return sm.Model(c["wide"], c["fmt"], c["N"], c["F"], w, P)


def run_spectrum(c, ctx, want):
    """the host form, then the device form into a buffer full of the drawn byte"""
    eng = ctx.eng
    s = capi.Spectrum(eng, c["N"], n_sources=c["n_src"], window=c["window"], sample_format=c["fmt"])
    bad = differs("host form: power", s.run(c["wide"], c["F"]), want)
    if bad is None:
        wide = np.ascontiguousarray(c["wide"])
        d_in, d_out = eng.dev_alloc(wide.nbytes), eng.dev_alloc(want.nbytes)
        eng.dev_upload(d_in, wide.view(np.uint8))
        eng.dev_upload(d_out, np.full(want.nbytes, c["fill"], np.uint8))
        s.run_device(d_in, wide.shape[1], c["F"], d_out)
        eng.synchronize()
        bad = differs("device form: power", eng.dev_download(d_out, want.nbytes, np.uint32).reshape(want.shape), want)
        eng.dev_free(d_in)
        eng.dev_free(d_out)
    s.close()
    return bad


def spectrum_case(rng, ctx, gpu=True):
    c = draw_spectrum(rng)
    want = spectrum_model(c, ctx.P).power()
    ctx.count("spectrum cases")
    bad = run_spectrum(c, ctx, want) if gpu else None
    return None if bad is None else "spectrum case: %s\n  %s" % (describe_spectrum(c), bad)


# ---------------------------------------------------------------------------------------------------- detector

def draw_detect_cfg(rng, N=None):
    N = int(pick(rng, N_SET)) if N is None else N
    Q = edge_or(rng, (256, 257, 512, 2048, 2 ** 24), 256, 2 ** 24, log=True)
    d = edge_or(rng, (0, 1, 2, N // 4), 0, N // 4, log=True) if rng.random() < 0.8 else int(rng.integers(0, 6))
    g = edge_or(rng, (0, 1, 2, 8, 63, 64), 0, 64) if rng.random() < 0.6 else int(rng.integers(0, 5))
    m = edge_or(rng, (1, 2, 3, 4, 64, 65, N), 1, N, log=True) if rng.random() < 0.4 else int(rng.integers(1, 7))
    K = edge_or(rng, (1, 2, 3, N // 2), 1, N // 2, log=True) if rng.random() < 0.7 else int(rng.integers(1, 9))
    rank = edge_or(rng, (0, 1, N // 4, N // 2, N - 2, N - 1), 0, N - 1)
    cfg = dm.Cfg(N, rank, Q, d, g, m, K)
    dm.check_cfg(cfg)
    return cfg


def draw_noise(rng, N):
    style = pick(rng, ("zeros", "one value", "one byte", "near 2^32", "sparse", "uniform", "uniform", "uniform"))
    if style == "zeros":
        p = np.zeros(N, np.int64)
    elif style == "one value":
        p = np.full(N, int(2.0 ** rng.uniform(0, 32)) - 1, np.int64)
    elif style == "one byte":
        by = 8 * int(rng.integers(0, 4))
        p = (int(rng.integers(0, 2 ** 32)) & ~(0xff << by)) | (rng.integers(0, 256, N) << by)
    elif style == "near 2^32":
        p = M32 - rng.integers(0, int(2.0 ** rng.uniform(0, 20)) + 1, N)
    elif style == "sparse":
        p = np.where(rng.random(N) < 0.2, rng.integers(1, int(2.0 ** rng.uniform(1, 12)) + 1, N), 0)
    else:
        p = rng.integers(0, int(2.0 ** rng.uniform(1, 32)), N)
    return style, p.astype(np.int64)


def draw_row(rng, cfg):
    """(what, the row): floor noise, the bins above the noise's own threshold cut down to it in most rows, and planted runs"""
    N, g, m, d = cfg.n_bins, cfg.bridge, cfg.min_width, cfg.dc_guard
    style, p = draw_noise(rng, N)
    f = int(np.sort(p)[cfg.floor_rank])
    T = min(M32, (max(f, 1) * cfg.ratio_q8) >> 8)
    quiet = rng.random() < 0.7
    cold = np.minimum(p, T)                                # (values above the floor only: the floor stays what it was)
    if quiet:
        p = cold.copy()
    if T >= M32 or rng.random() < 0.08:
        return style + " bare", p.astype(np.uint32)
    hi = min(M32, max(T + 1, int((T + 1) * 2.0 ** rng.uniform(0.01, 8))))

    def values(n):
        vs = int(rng.integers(0, 5))
        if vs == 0:
            v = np.full(n, int(rng.integers(T + 1, hi + 1)), np.int64)      # equal peaks all along
        elif vs == 1:
            v = np.full(n, M32, np.int64)
        else:
            v = rng.integers(T + 1, hi + 1, n)
            if vs == 2 and n >= 2:                          # the peak twice, as far apart as the run allows
                v[0] = v[-1] = int(v.max()) if rng.random() < 0.5 else M32
            if vs == 3:
                v[rng.integers(0, n, 2)] = M32
        return v

    lengths = (m - 1, m, m + 1, 1, 2, 3, 63, 64, 65, 129, 130, 200)
    pos = int(pick(rng, (0, 0, 1, 62, 63, 64))) if rng.random() < 0.5 else int(rng.integers(0, N))
    stop = rng.uniform(0.03, 0.3)
    while pos < N:
        L = max(1, int(pick(rng, lengths))) if rng.random() < 0.7 else int(rng.integers(1, 10))
        if rng.random() < 0.35:                             # the end at 62 .. 65 modulo 64
            want_end = int(pick(rng, (62, 63, 0, 1)))
            L += (want_end - (pos + L - 1)) % 64
        end = min(pos + L, N)
        if rng.random() < 0.1:
            end = N                                         # up to the row's last bin
        hot = np.ones(end - pos, bool)
        if g >= 1 and end - pos >= 3 and rng.random() < 0.5:          # holes of up to g bins, some over a multiple of 64
            for _ in range(int(rng.integers(1, 4))):
                width = int(rng.integers(1, g + 1)) if rng.random() < 0.6 else g
                seam = (pos // 64 + 1) * 64 + 64 * int(rng.integers(0, max(1, (end - pos) // 64)))
                if rng.random() < 0.5 and pos < seam - width and seam + width < end:
                    a = seam - int(rng.integers(0, width + 1)) - pos
                else:
                    a = int(rng.integers(1, end - pos - 1))
                hot[a:min(a + width, end - pos - 1)] = False
            hot[0] = hot[-1] = True
        k = pos + np.flatnonzero(hot)
        p[k] = values(len(k))
        p[pos + np.flatnonzero(~hot)] = cold[pos + np.flatnonzero(~hot)]
        if rng.random() < stop:
            break
        gap = int(pick(rng, (g, g + 1, g + 1, g + 2, g + 2))) if rng.random() < 0.75 else int(rng.integers(g + 1, g + 130))
        p[end:end + gap] = cold[end:end + gap]
        pos = end + max(gap, 1)
        if rng.random() < 0.25:                             # the next start at 62 .. 65 modulo 64
            pos += (int(pick(rng, (62, 63, 0, 1))) - pos) % 64
    if rng.random() < 0.3:                                  # a run over the guard, its guard bins as strong as the rest or more
        a, b = d + int(rng.integers(0, 4)), d + int(rng.integers(0, 4))
        k = np.arange(max(N // 2 - a, 0), min(N // 2 + b + 1, N))
        p[k] = values(len(k))
        if rng.random() < 0.5:
            p[N // 2] = M32
    return style, p.astype(np.uint32)


def draw_detect(rng):
    cfg = draw_detect_cfg(rng)
    n_rows = int(pick(rng, ROW_EDGES)) if rng.random() < 0.5 else int(rng.integers(1, 71))
    n_rows = min(n_rows, max(9, 32768 // cfg.n_bins))
    what, power = [], np.zeros((n_rows, cfg.n_bins), np.uint32)
    for i in range(n_rows):
        w, power[i] = draw_row(rng, cfg)
        what.append(w)
    return dict(cfg=cfg, power=power, what=sorted(set(what)), fill=int(rng.integers(0, 256)))


def describe_detect(c):
    return "%s rows %d noise %s fill 0x%02x" % (c["cfg"], len(c["power"]), "/".join(c["what"]), c["fill"])


def _detector(eng, cfg):
    return capi.Detector(eng, cfg.n_bins, cfg.floor_rank, cfg.ratio_q8, cfg.dc_guard, cfg.bridge, cfg.min_width, cfg.max_detections)


def run_detect(c, ctx, want):
    """the host form, then the device form into buffers full of the drawn byte: both arrays in full"""
    eng, cfg, power = ctx.eng, c["cfg"], c["power"]
    n_rows, K = len(power), cfg.max_detections
    d = _detector(eng, cfg)
    rows, det = d.run(power)
    bad = differs("host form: rows", rows, want[0]) or differs("host form: det", det, want[1])
    if bad is None:
        d_in, d_rows, d_det = eng.dev_alloc(power.nbytes), eng.dev_alloc(16 * n_rows), eng.dev_alloc(32 * n_rows * K)
        eng.dev_upload(d_in, power.view(np.uint8))
        eng.dev_upload(d_rows, np.full(16 * n_rows, c["fill"], np.uint8))
        eng.dev_upload(d_det, np.full(32 * n_rows * K, c["fill"], np.uint8))
        d.run_device(d_in, n_rows, d_rows, d_det)
        eng.synchronize()
        rows = eng.dev_download(d_rows, 16 * n_rows).view(capi.DETECT_ROW)
        det = eng.dev_download(d_det, 32 * n_rows * K).view(capi.DETECTION).reshape(n_rows, K)
        bad = differs("device form: rows", rows, want[0]) or differs("device form: det", det, want[1])
        for p in (d_in, d_rows, d_det):
            eng.dev_free(p)
    d.close()
    return bad


def detect_case(rng, ctx, gpu=True):
    c = draw_detect(rng)
    want = dm.detect(c["power"], c["cfg"])
    ctx.count("detect cases")
    ctx.count("detect rows", len(c["power"]))
    bad = run_detect(c, ctx, want) if gpu else None
    return None if bad is None else "detect case: %s\n  %s" % (describe_detect(c), bad)


# ---------------------------------------------------------------------------------------------------- tracker

def draw_track_cfg(rng):
    n_src, N = int(rng.integers(1, 4)), int(pick(rng, N_SET))
    S = edge_or(rng, (1, 2, 63, 64), 1, 64)
    K = edge_or(rng, (1, 64, 65, 128, N // 2), 1, min(N // 2, 140))
    G = edge_or(rng, (0, 1, 255, 256, 512, 1024), 0, min(256 * N - 1, 4096), log=True)
    H = edge_or(rng, (1, 2, 3), 1, 6) if rng.random() < 0.95 else 255
    B = edge_or(rng, (0, 1, 2), 0, 4) if rng.random() < 0.95 else 65535
    A = edge_or(rng, (1, 64, 128, 255, 256), 1, 256)
    bias = edge_or(rng, (0, 1, 2 ** 31, M32), 0, M32)
    edges = tuple(sorted(int(e) for e in (rng.integers(1, 8, 3) if rng.random() < 0.7 else rng.integers(1, N + 2, 3))))
    cfg = tm.Cfg(n_src, N, K, S, G, H, B, A, bias, edges)
    tm.check_cfg(cfg)
    return cfg


def _records(cands, N):
    """(centroid, width, peak) candidates -> the detector's kind of records: ascending, disjoint, the centroid inside"""
    out, prev_last = [], -1
    for cq, w, peak in sorted(cands):
        b = cq >> 8
        first = max(b - (w - 1) // 2, 0)
        last = min(first + w - 1, N - 1)
        if first <= prev_last or not 0 <= cq < 256 * N:
            continue
        out.append((first, last, (first + last) // 2, peak, peak * (last - first + 1), cq, last - first + 1))
        prev_last = last
    return out


def draw_track(rng):
    """The configuration, the detector arrays of every block, the script of calls - and the model's arrays, since the script
    is drawn block by block against the model's slots."""
    cfg = draw_track_cfg(rng)
    n_src, N, K, S, G = cfg.n_sources, cfg.n_bins, cfg.max_detections, cfg.n_slots, cfg.gate_q8
    long_life, crowd = rng.random() < 0.06, False          # a track that outlives 255 hits
    if long_life:
        cfg = cfg._replace(n_sources=1, n_slots=min(S, 2), hold_blocks=min(cfg.hold_blocks, 4))
        n_src, S = 1, cfg.n_slots
        n_blocks, n_st = 257 + int(rng.integers(0, 40)), 1
    else:
        n_blocks = int(rng.integers(1, 25))
        n_st = int(rng.integers(1, -(-3 * S // 2) + 1))
        crowd = K > 64 and rng.random() < 0.5              # more than one trip of 64 records
        if crowd:
            n_st = int(rng.integers(70, 111))
            if rng.random() < 0.7:                          # mostly with slots for most of them and a gate they can tie in
                cfg = cfg._replace(n_slots=int(pick(rng, (63, 64, 64, int(rng.integers(40, 65))))),
                                   gate_q8=G if G >= 64 else int(pick(rng, (256, 512, 1024))))
                S, G = cfg.n_slots, cfg.gate_q8
        n_st = min(n_st, N // 2)
        while n_src * n_blocks * S * min(n_st, K) > TRACK_BUDGET and n_blocks > 2:
            n_blocks -= 1
    stations = []
    on0 = float(rng.uniform(0.25, 0.6)) if crowd else 0.6  # (a crowd gathers over the first blocks: its tracks lie all over the band)
    for j in range(n_src):
        bins = np.sort(rng.choice(N, n_st, replace=False))
        widths = (1, 1, 1, 2) if crowd else (1, 1, 2, 3, 5)
        stations.append([dict(cq=256 * int(b) + int(rng.integers(0, 256)), home=None, w=int(pick(rng, widths)), on=rng.random() < on0,
                              peak=int(rng.integers(1, 2 ** 32))) for b in bins])
        if crowd and G >= 2:                               # twins 2 G' <= 2 G apart in the upper half: ties past record 64
            for st in list(stations[j][n_st // 2:]):
                if rng.random() < 0.5 and st["cq"] + G < 256 * N:
                    stations[j].append(dict(st, cq=st["cq"] + 2 * int(rng.integers(min(256, G), G + 1)), w=1))
    reset_at = int(rng.integers(1, n_blocks)) if n_blocks > 1 and rng.random() < 0.3 else None
    cuts = sorted(set(int(x) for x in rng.integers(1, n_blocks, int(rng.integers(0, 4))))) if n_blocks > 1 and rng.random() < 0.6 else []
    if reset_at is not None and reset_at not in cuts:
        cuts = sorted(cuts + [reset_at])                   # (a reset lies between two calls)
    p_off, p_on = float(rng.uniform(0.02, 0.3)), float(rng.uniform(0.05, 0.5))
    if crowd:
        p_off, p_on = float(rng.uniform(0.01, 0.08)), float(rng.uniform(0.3, 0.6))
    raw = rng.integers(0, 256, (n_src, n_blocks, K, 32), dtype=np.uint8)       # garbage past D
    det = np.ascontiguousarray(raw).view(dm.DET_DTYPE).reshape(n_src, n_blocks, K)
    rows = np.zeros((n_src, n_blocks), dm.ROW_DTYPE)
    rows["floor"], rows["threshold"] = 100, 800
    model = tm.Tracker(cfg)
    slots, blocks = [], []
    for b in range(n_blocks):
        if b == reset_at:
            model.reset()
        for j in range(n_src):
            cands = []
            for st in stations[j]:
                if not long_life:
                    st["on"] = (rng.random() >= p_off) if st["on"] else (rng.random() < p_on)
                if not st["on"]:
                    continue
                if long_life:                               # never far from where it was born: one track all along
                    st["home"] = st["cq"] if st["home"] is None else st["home"]
                    st["cq"] = st["home"] - int(rng.integers(0, G // 3 + 1))
                r = rng.random()
                step = 0
                if not long_life and r >= 0.3:
                    step = int(rng.integers(-G // 3 - 1, G // 3 + 2)) if r < 0.9 else int(pick(rng, (-G, G, -G - 1, G + 1)))
                st["cq"] = min(max(st["cq"] + step, 0), 256 * N - 1)
                w = st["w"] + (int(rng.integers(0, 4)) if rng.random() < 0.2 else 0)
                cands.append((st["cq"], w, st["peak"] if rng.random() < 0.7 else int(rng.integers(1, 2 ** 32))))
            live = sorted(x["centre_q8"] for x in model.slots[j] if x["state"] != tm.FREE)
            n_special = 0 if long_life else int(rng.integers(2, 12)) if crowd else int(rng.integers(0, 3))
            pairs = [(lo, hi) for lo, hi in zip(live, live[1:]) if lo < hi <= lo + 2 * G and (lo + hi) % 2 == 0]
            for _ in range(n_special if live else 0):
                kind = pick(rng, ("G", "G1", "mid", "mid", "mid", "dup"))
                # (mostly a crowd's upper half: records past the first trip of 64)
                i = int(rng.integers(len(live) // 2 if crowd and rng.random() < 0.7 else 0, len(live)))
                if kind == "G":
                    c = live[i] + int(pick(rng, (-G, G)))
                elif kind == "G1":
                    c = live[i] + int(pick(rng, (-G - 1, G + 1)))
                elif kind == "dup":
                    c = live[i] + int(rng.integers(-G // 2 - 1, G // 2 + 2))
                else:                                       # half way between two neighbouring tracks, both in the gate
                    if not pairs:
                        continue
                    lo, hi = pairs[int(rng.integers(len(pairs) // 2 if crowd and rng.random() < 0.7 else 0, len(pairs)))]
                    c = (lo + hi) // 2
                    if rng.random() < 0.7:                  # the lower track's own station fades for this block: when the
                        cands = [x for x in cands if not lo - G <= x[0] < c]      # detection's turn comes both tracks are to be had
                cands.append((c, 1, int(rng.integers(1, 2 ** 32))))
            if not long_life and rng.random() < (0.5 if crowd else 0.15) and live and G >= 2:
                # a station born 2 G' <= 2 G above a track: once both are tracks, a detection can lie half way between them
                i = int(rng.integers(len(live) // 2 if crowd else 0, len(live)))
                twin = dict(cq=live[i] + 2 * int(rng.integers(min(256, G), G + 1)), home=None, w=1, on=True,
                            peak=int(rng.integers(1, 2 ** 32)))
                if twin["cq"] < 256 * N:
                    stations[j].append(twin)
                    cands.append((twin["cq"], 1, twin["peak"]))
            recs = _records(cands, N)
            n_found = len(recs)
            if len(recs) >= K and rng.random() < 0.5:
                n_found = int(pick(rng, (K + 1, 2 * K, len(recs) + 5, M32)))
            for i, r in enumerate(recs[:K]):
                det[j, b, i] = r
            rows[j, b]["n_found"] = n_found
            rows[j, b]["n_hot_bins"] = sum(r[6] for r in recs)
        s, bl = model.run(rows[:, b:b + 1], det[:, b:b + 1])
        slots.append(s)
        blocks.append(bl)
    calls, b0 = [], 0
    for cut in cuts + [n_blocks]:
        if b0 == reset_at:
            calls.append(("reset",))
        calls.append(("run", b0, cut))
        b0 = cut
    return dict(cfg=cfg, n_blocks=n_blocks, rows=rows, det=det, calls=calls, n_st=n_st, long_life=long_life,
                want=(np.concatenate(slots, axis=1), np.concatenate(blocks, axis=1)), fill=int(rng.integers(0, 256)))


def describe_track(c):
    return "%s blocks %d stations %d calls %s fill 0x%02x" % (c["cfg"], c["n_blocks"], c["n_st"], c["calls"], c["fill"])


def track_script(c, tracker):
    """the case's calls on anything with run(rows, det) and reset(): (slots, blocks) of all the blocks, in order"""
    slots, blocks = [], []
    for op in c["calls"]:
        if op[0] == "reset":
            tracker.reset()
        else:
            s, b = tracker.run(np.ascontiguousarray(c["rows"][:, op[1]:op[2]]), np.ascontiguousarray(c["det"][:, op[1]:op[2]]))
            slots.append(s)
            blocks.append(b)
    return np.concatenate(slots, axis=1), np.concatenate(blocks, axis=1)


def track_model(c, defects=()):
    return track_script(c, tm.Tracker(c["cfg"], defects))


def _tracker(eng, cfg):
    return capi.Tracker(eng, cfg.n_bins, cfg.n_sources, cfg.max_detections, cfg.n_slots, cfg.gate_q8, cfg.open_hits, cfg.hold_blocks,
                        cfg.alpha_q8, cfg.inc_bias, cfg.class_edge)


class _DeviceTracker:
    """run(rows, det) through iqd_track_run_device into buffers full of the drawn byte"""

    def __init__(self, eng, t, cfg, fill):
        self.eng, self.t, self.cfg, self.fill = eng, t, cfg, fill

    def reset(self):
        self.t.reset()

    def run(self, rows, det):
        cfg, eng = self.cfg, self.eng
        nb = rows.shape[1]
        n_rows = cfg.n_sources * nb
        sizes = (16 * n_rows, 32 * n_rows * cfg.max_detections, 32 * n_rows * cfg.n_slots, 16 * n_rows)
        ptrs = [eng.dev_alloc(n) for n in sizes]
        eng.dev_upload(ptrs[0], rows.view(np.uint8))
        eng.dev_upload(ptrs[1], det.view(np.uint8))
        eng.dev_upload(ptrs[2], np.full(sizes[2], self.fill, np.uint8))
        eng.dev_upload(ptrs[3], np.full(sizes[3], self.fill, np.uint8))
        self.t.run_device(ptrs[0], ptrs[1], nb, ptrs[2], ptrs[3])
        eng.synchronize()
        slots = eng.dev_download(ptrs[2], sizes[2]).view(capi.TRACK_SLOT).reshape(cfg.n_sources, nb, cfg.n_slots)
        blocks = eng.dev_download(ptrs[3], sizes[3]).view(capi.TRACK_BLOCK).reshape(cfg.n_sources, nb)
        for p in ptrs:
            eng.dev_free(p)
        return slots, blocks


def run_track(c, ctx, want):
    """the script in the host form and, on a second tracker, in the device form; get_state after the last call"""
    eng, cfg = ctx.eng, c["cfg"]
    bad = None
    for form in ("host", "device"):
        t = _tracker(eng, cfg)
        got = track_script(c, t if form == "host" else _DeviceTracker(eng, t, cfg, c["fill"]))
        bad = differs(form + " form: slots", got[0], want[0]) or differs(form + " form: blocks", got[1], want[1])
        for j in range(cfg.n_sources):
            bad = bad or differs(form + " form: get_state of source %d" % j, t.state(j), want[0][j, -1])
        t.close()
        if bad is not None:
            break
    return bad


def track_case(rng, ctx, gpu=True):
    c = draw_track(rng)
    want = track_model(c)
    assert want[0].tobytes() == c["want"][0].tobytes() and want[1].tobytes() == c["want"][1].tobytes()   # the draw's own run
    ctx.count("track cases")
    ctx.count("track blocks", c["n_blocks"] * c["cfg"].n_sources)
    bad = run_track(c, ctx, want) if gpu else None
    return None if bad is None else "track case: %s\n  %s" % (describe_track(c), bad)


# ---------------------------------------------------------------------------------------------------- chain

def draw_chain(rng):
    N = int(pick(rng, N_SET))
    fmt = pick(rng, ("u8", "s8"))
    n_src = int(rng.integers(1, 4))
    blocks = int(rng.integers(6, 25))
    F = int(pick(rng, (1, 2, 3, 4, 8, 16)))
    while N * N * F * n_src * blocks > SPECTRUM_BUDGET // 2:
        if F > 1:
            F = max(1, F // 2)
        elif n_src > 1:
            n_src -= 1
        else:
            blocks -= 1
    wkind, window = draw_window(rng, N) if rng.random() < 0.3 else ("default", None)
    n = N * F * blocks
    wide = []
    for j in range(n_src):
        st = []
        for i in range(int(rng.integers(1, 5))):
            edges = np.sort(rng.integers(0, n + 1, 4))
            st.append({"offset": float(rng.uniform(-0.45, 0.45)) * RATE, "kind": pick(rng, ("am", "usb", "fm")),
                       "amplitude": float(2.0 ** rng.uniform(2.5, 5.3)), "tone": 700.0 + 300 * i,
                       "on": [(int(edges[0]), int(edges[1])), (int(edges[2]), int(edges[3]))]})
        wide.append(synth.wideband(n, RATE, st, seed=int(rng.integers(1 << 30)), sigma=float(pick(rng, (0.5, 1.0, 2.0, 4.0)))))
    u8 = np.ascontiguousarray(np.stack(wide))
    K = int(pick(rng, (1, 2, 4, 16, 16)))
    dcfg = dm.Cfg(N, int(pick(rng, (N // 2, N // 4, N // 2 + 7))), int(pick(rng, (1024, 2048, 4096))), int(pick(rng, (0, 1, 2))),
                  int(pick(rng, (0, 2, 8, 16))), int(pick(rng, (1, 2, 3))), K)
    dm.check_cfg(dcfg)
    tcfg = tm.Cfg(n_src, N, K, int(pick(rng, (1, 2, 4, 8, 64))), int(pick(rng, (256, 512, 1024))), int(pick(rng, (1, 2, 3))),
                  int(pick(rng, (0, 1, 2))), int(pick(rng, (64, 128, 256))), int(pick(rng, (0, 2 ** 31, 12345))),
                  (max(N // 64, 1) + 1, max(N // 16, 2), max(N // 4, 3)))
    tm.check_cfg(tcfg)
    cut = int(rng.integers(1, blocks)) if rng.random() < 0.5 else None
    return dict(N=N, fmt=fmt, n_src=n_src, blocks=blocks, F=F, wkind=wkind, window=window, dcfg=dcfg, tcfg=tcfg, cut=cut,
                wide=u8 if fmt == "u8" else (u8 ^ 0x80).view(np.int8))


def describe_chain(c):
    return "N %d %s window %s F %d sources %d blocks %d cut %s %s %s" % (
        c["N"], c["fmt"], c["wkind"], c["F"], c["n_src"], c["blocks"], c["cut"], c["dcfg"], c["tcfg"])


def chain_model(c, P):
    """the three models chained: (power, rows, det, slots, blocks)"""
    N, nb, n_src, K = c["N"], c["blocks"], c["n_src"], c["dcfg"].max_detections
    power = spectrum_model(dict(c), P).power()
    rows, det = dm.detect(power.reshape(-1, N), c["dcfg"])
    rows, det = rows.reshape(n_src, nb), det.reshape(n_src, nb, K)
    slots, blocks = tm.Tracker(c["tcfg"]).run(rows, det)
    return power, rows, det, slots, blocks


def run_chain(c, ctx, want):
    """Spectrum, Detector, Tracker queued back to back per call, one synchronise after the last call; every call's arrays
    lie in the context's buffers, one region per call, with whatever earlier cases left there around them"""
    eng, N, F, n_src, nb = ctx.eng, c["N"], c["F"], c["n_src"], c["blocks"]
    K, S = c["dcfg"].max_detections, c["tcfg"].n_slots
    s = capi.Spectrum(eng, N, n_sources=n_src, window=c["window"], sample_format=c["fmt"])
    d, t = _detector(eng, c["dcfg"]), _tracker(eng, c["tcfg"])
    per_block = dict(wide=2 * N * F, power=4 * N, rows=16, det=32 * K, slots=32 * S, blocks=16)
    ptr = {k: ctx.buffer(k, v * n_src * nb) for k, v in per_block.items()}
    calls = [(0, nb)] if c["cut"] is None else [(0, c["cut"]), (c["cut"], nb)]
    launches = eng.stats()["device_launches"]
    for b0, b1 in calls:
        piece = np.ascontiguousarray(c["wide"][:, b0 * 2 * N * F:b1 * 2 * N * F])
        eng.dev_upload(ptr["wide"] + n_src * b0 * per_block["wide"], piece.view(np.uint8))
    for b0, b1 in calls:
        at = {k: ptr[k] + n_src * b0 * v for k, v in per_block.items()}
        n = b1 - b0
        s.run_device(at["wide"], n * per_block["wide"], F, at["power"])
        d.run_device(at["power"], n_src * n, at["rows"], at["det"])
        t.run_device(at["rows"], at["det"], n, at["slots"], at["blocks"])
    queued = eng.stats()["device_launches"] - launches
    eng.synchronize()
    dtypes = dict(power=np.uint32, rows=capi.DETECT_ROW, det=capi.DETECTION, slots=capi.TRACK_SLOT, blocks=capi.TRACK_BLOCK)
    bad = None if queued == 3 * len(calls) else "%d launches for %d calls" % (queued, len(calls))
    for i, name in enumerate(("power", "rows", "det", "slots", "blocks")):
        parts = []
        for b0, b1 in calls:
            raw = eng.dev_download(ptr[name] + n_src * b0 * per_block[name], n_src * (b1 - b0) * per_block[name])
            parts.append(raw.view(dtypes[name]).reshape((n_src, b1 - b0) + want[i].shape[2:]))
        bad = bad or differs("chained: " + name, np.concatenate(parts, axis=1), want[i])
    for j in range(n_src):
        bad = bad or differs("chained: get_state of source %d" % j, t.state(j), want[3][j, -1])
    for o in (t, d, s):
        o.close()
    return bad


def chain_case(rng, ctx, gpu=True):
    c = draw_chain(rng)
    want = chain_model(c, ctx.P)
    ctx.count("chain cases")
    ctx.count("chain opened", int((want[4]["n_opened_closed"] & 0xffff).sum()))
    ctx.count("chain closed", int((want[4]["n_opened_closed"] >> 16).sum()))
    ctx.count("chain detections", int(np.minimum(want[1]["n_found"], c["dcfg"].max_detections).sum()))
    bad = run_chain(c, ctx, want) if gpu else None
    return None if bad is None else "chain case: %s\n  %s" % (describe_chain(c), bad)


KINDS = {"spectrum": spectrum_case, "detect": detect_case, "track": track_case, "chain": chain_case}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--kind", choices=sorted(KINDS), required=True)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--case", type=int, default=None, help="run this one case of the seed again")
    ap.add_argument("--model-only", action="store_true", help="draw and run the models, no GPU")
    a = ap.parse_args()
    ctx = Context(gpu=not a.model_only)
    fn = KINDS[a.kind]
    t0 = time.time()
    todo = range(a.cases) if a.case is None else [a.case]
    for i in todo:
        if i and i % 200 == 0:
            print("band_fuzz: %d %s cases so far, %.0f s" % (i, a.kind, time.time() - t0), flush=True)
        bad = fn(case_rng(a.seed, i), ctx, gpu=not a.model_only)
        if bad is not None:
            print("MISMATCH in case %d of seed %d: %s" % (i, a.seed, bad))
            print("again: python tools/band_fuzz.py --kind %s --seed %d --case %d" % (a.kind, a.seed, i))
            ctx.close()
            sys.exit(1)
    print("band_fuzz: %d %s cases of seed %d identical to the model in %.0f s (%s)"
          % (len(todo), a.kind, a.seed, time.time() - t0, ", ".join("%d %s" % (v, k) for k, v in ctx.stats.items())))
    ctx.close()


if __name__ == "__main__":
    main()
