"""Diagnostic: randomized channelizer-vs-model runs on an MI355X (include/iqdemod.h: iqd_channelizer_*, bit for bit
against tests/chan_model.py; scanner-driven channels against tests/chan_scan_model.py on oracle chains).

    python tools/chan_fuzz.py [cases] [seed]

Bound by a case count, so that a seed is the same cases on every machine.  One case in eight is a scan case
(FUZZ_SCAN=1: every case, FUZZ_SCAN=0: none), and about one in six of the rest a fractional one (decimation P / Q, Q = 2,
4, 8, against tests/chan_frac_model.py; FUZZ_FRAC=1: every such case, FUZZ_FRAC=0: none - a case kind is decided by the
first draw of the case, so that a kept generator state replays the same kind).  On the first difference it prints the whole configuration, leaves the
generator state of that case in fuzz_out/chan_fuzz_fail_state.json (FUZZ_STATE=<path>: there) and exits non-zero;
FUZZ_REPLAY=<that file> python tools/chan_fuzz.py  runs that one case again.

About one case in ten is a survey case (FUZZ_SURVEY=1: every case, FUZZ_SURVEY=0: none): a plain or a fractional case with
a band survey (iqd_channelizer_survey*, against tests/chan_survey_model.py) drawn before some of its calls, each followed by
the call itself, so that a survey that moved the channelizer's state shows in the rows.

Gain cases (channels that follow their engine channel's IF gain, iqd_channelizer_follow_gain, against
tests/chan_gain_model.py on oracle chains) are drawn only when asked: FUZZ_GAIN=1 makes every case one, and nothing else
draws them, so that a seed without it is the cases it always was.

Track cases (channels that follow the slots of a track table, iqd_channelizer_follow_tracks, against
tests/chan_track_model.py) are drawn only when asked as well: FUZZ_TRACK=1 makes every case one.

Format cases (signed captures: sample_format "s8" / "s16", chz_fmt_kernel, against tests/chan_fmt_model.py) are drawn only
when asked as well: FUZZ_FMT=1 makes every case one.  Such a case is drawn without a GPU (draw_fmt) and then run (run_fmt):
M, taps, sources, channels, calls and the operator's steps as in a plain case, the long calls sized by
iqd_channelizer_window_outputs of the format, inputs of the format's dtype (full range, small with a live low byte, on the
rails, constant, carriers), a share with a stage-a half point planted on channel 0 and a share on the taps' limit with
sign-matched rail input (sat16; Lo outside int32).  tests/test_chan_fmt_fuzz_host.py holds the fixed slice SLICES["fmt"]
to the defects of tests/chan_fmt_model.py before tests/test_gpu_chan_fmt_fuzz.py runs it.

A plain case is drawn without a GPU (draw_plain) and then run (run_plain), so that a CPU test can hold the fixed slices
of tests/test_gpu_chan_fuzz.py to the mutants of tests/chan_mutants.py before they go to the GPU (first_channel_kills)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                     # noqa: E402
from rtlsdrdiags_amd import capi, synth                # noqa: E402
from tests import chan_fmt_cases as fc                 # noqa: E402
from tests import chan_fmt_model as sfm                # noqa: E402
from tests import chan_frac_model as fm                # noqa: E402
from tests import chan_gain_model as gm                # noqa: E402
from tests import chan_model as cm                     # noqa: E402
from tests import chan_mutants as mu                   # noqa: E402
from tests import chan_scan_model as sm                # noqa: E402
from tests import chan_survey_model as svm             # noqa: E402
from tests import chan_track_cases as tkc              # noqa: E402
from tests import chan_track_model as tkm              # noqa: E402

K_EDGES = (1, 31, 32, 33, 255, 256, 257, 1023, 1024)
INC_EDGES = (0, 1, 2 ** 31, 2 ** 31 - 1, 2 ** 32 - 1)
BOUND_SUM = (2 ** 31 - 256) // 256
SLICES = {"plain": ((9101, 150), (9102, 150)), "scan": (9103, 40),   # (seed, cases): tests/test_gpu_chan_fuzz.py's
          "survey": (9104, 40),                                       # tests/test_gpu_chan_survey_fuzz.py's
          "gain": (9105, 24),                                         # tests/test_gpu_chan_gain_fuzz.py's
          "fmt": (9106, 36),                                          # tests/test_gpu_chan_fmt_fuzz.py's
          "track": (9107, 24)}                                        # tests/test_gpu_chan_track_fuzz.py's
MODEL_BUDGET = 4e7        # tap x wideband-sample products the model may spend per case (chan_model convolves at the
#                           wide rate: K M outputs per channel); fewer channels are compared when a case is past it


def t_max(M, K):
    """outputs per window of the kernels (iqd_chan.cpp: chz_launch)"""
    kp = (K + 31) // 32 * 32
    return min(1024, (16384 - kp) // M) // 64 * 64


def draw_taps(rng, M):
    """(taps argument, h): None -> the default prototype"""
    if rng.random() < 0.5:
        K = int(rng.integers(1, 1025))
    else:
        K = int(rng.choice(K_EDGES + (0,)))
        if K == 0:
            return None, capi.channelizer_default_taps(M)
    smax = min(32639, BOUND_SUM // K)
    if rng.random() < 0.06:                               # exactly at the bound (K >= 258), else the largest taps
        h = np.full(K, smax, np.int64) * rng.choice([-1, 1], K)
        if K * 32639 >= BOUND_SUM:
            h[:BOUND_SUM - K * smax] += np.sign(h[:BOUND_SUM - K * smax])
        return h.astype(np.int16), h.astype(np.int16)
    s = int(2.0 ** rng.uniform(3, np.log2(smax)))
    h = rng.integers(-s, s + 1, K).astype(np.int16)
    if rng.random() < 0.25:                               # a few taps at the extremes, whatever the scale of the rest
        at = rng.choice(K, min(K, 3), replace=False)
        h[at] = rng.choice([-32639, 32639], len(at))
        if np.abs(h.astype(np.int64)).sum() > BOUND_SUM:
            h[at] = 0
    return h, h


def draw_input(rng, M, n_samples):
    kind = int(rng.integers(0, 5))
    seed = int(rng.integers(1 << 30))
    if kind == 0:
        return "white", synth.white_u8(n_samples, seed)
    if kind == 1:
        return "rails", synth.rails_u8(n_samples, seed)
    if kind == 2:
        amp = int(2.0 ** rng.uniform(0, 5))
        return "low %d" % amp, (128 + np.random.default_rng(seed).integers(-amp, amp + 1, 2 * n_samples)).astype(np.uint8)
    if kind == 3:
        fs = 256000.0 * M
        st = [{"offset": float(rng.uniform(-0.45, 0.45)) * fs, "kind": ("fm", "am", "usb")[i % 3],
               "amplitude": float(2.0 ** rng.uniform(1, 5.5)), "tone": 1000.0 + 300 * i,
               "on": [(int(a), int(a) + int(rng.integers(1, n_samples + 1)))
                      for a in rng.integers(0, n_samples, 2)]} for i in range(int(rng.integers(1, 4)))]
        return "carriers", synth.wideband(n_samples, fs, st, seed=seed, sigma=float(rng.choice([0.0, 1.0, 4.0])))
    return "constant", np.tile(rng.integers(0, 256, 2).astype(np.uint8), n_samples)


def draw_count(rng):
    r = rng.random()
    if r < 0.4:
        return int(rng.integers(1, 4))
    if r < 0.65:
        return int(rng.integers(7, 10))
    if r < 0.87:
        return int(rng.integers(63, 66))
    return int(rng.integers(100, 400))


def draw_inc(rng):
    return int(rng.choice(INC_EDGES)) if rng.random() < 0.3 else int(rng.integers(0, 2 ** 32))


def draw_plain(rng):
    """One plain case, drawn without a GPU: the configuration, the wideband bytes and the script of calls and operator
    steps between them."""
    M = int(rng.integers(2, 65))
    taps, h = draw_taps(rng, M)
    K = len(h)
    n_src = int(rng.integers(1, 5))
    used = [s for s in range(n_src) if rng.random() < 0.7] or [int(rng.integers(0, n_src))]   # the rest: no channel
    n_ch = draw_count(rng)
    src = rng.choice(used, n_ch).astype(np.uint32)
    inc = np.array([draw_inc(rng) for _ in range(n_ch)], np.uint64)
    shift = rng.integers(0, 9, n_ch).astype(np.uint8)
    tm = t_max(M, K)
    calls, long_calls = [], 0
    for _ in range(int(rng.integers(1, 9))):
        r = rng.random()
        if r < 0.3:
            u = 1                                                       # the shortest call: 32 outputs
        elif r < 0.55:
            u = 2 * int(rng.integers(1, 6)) + 1                         # n_out % 64 == 32
        elif r < 0.8 or long_calls >= 2:
            u = 2 * int(rng.integers(1, 6))
        else:
            u = tm // 32 + int(rng.integers(1, 7))                      # several windows; odd: a 32-output tail
            long_calls += 1
        ops = []
        if calls and rng.random() < 0.5:
            what = int(rng.integers(0, 4))
            if what == 0:
                first = int(rng.integers(0, n_ch))
                n = int(rng.integers(1, min(4, n_ch - first) + 1))
                ops.append(("retune", first, [draw_inc(rng) for _ in range(n)], [int(v) for v in rng.integers(0, 9, n)]))
            elif what == 1:
                ops.append(("move", int(rng.integers(0, n_ch)), int(rng.integers(0, n_src))))
            elif what == 2:
                ops.append(("reset",))
            else:
                ops.append(("form",))
        calls.append({"units": u, "ops": ops})
    kinds, wide = [], []
    total = sum(c["units"] for c in calls) * 32 * M
    for s in range(n_src):
        k, w = draw_input(rng, M, total)
        kinds.append(k)
        wide.append(w)
    n_check = n_ch if n_ch <= 64 else 32
    work = 4.0 * K * M * sum(c["units"] for c in calls) * 32
    n_check = int(max(min(4, n_ch), min(n_check, MODEL_BUDGET // work)))
    check = np.arange(n_ch) if n_check == n_ch else np.unique(np.concatenate(
        [[0, n_ch - 1], rng.choice(n_ch, n_check, replace=False)]))
    return {"M": M, "K": K, "taps": taps, "h": h, "n_src": n_src, "n_ch": n_ch, "src": src, "inc": inc, "shift": shift,
            "calls": calls, "kinds": kinds, "wide": np.stack(wide), "check": check, "device_form": bool(rng.random() < 0.5)}


def describe(cfg):
    return ("M=%d K=%d (%s, sum|h|=%d) sources=%d (inputs %s) channels=%d calls(units of 64M bytes)=%r ops=%r "
            "src=%r inc=%r shift=%r" % (
                cfg["M"], cfg["K"], "default taps" if cfg["taps"] is None else "max|h|=%d" % np.abs(cfg["h"].astype(int)).max(),
                np.abs(cfg["h"].astype(np.int64)).sum(), cfg["n_src"], cfg["kinds"], cfg["n_ch"],
                [c["units"] for c in cfg["calls"]], [(i, c["ops"]) for i, c in enumerate(cfg["calls"]) if c["ops"]],
                cfg["src"].tolist()[:16], cfg["inc"].tolist()[:16], cfg["shift"].tolist()[:16]))


def walk(cfg):
    """The script, step by step: yields (call index, device form?, ops applied before it, the epoch's wideband bytes
    so far [n_src, bytes] (from the last reset), first output of this call in the epoch, outputs, src, inc, shift)."""
    M, unit = cfg["M"], 64 * cfg["M"]
    src, inc, shift = cfg["src"].copy(), cfg["inc"].copy(), cfg["shift"].copy()
    device, at, epoch0 = cfg["device_form"], 0, 0
    for i, call in enumerate(cfg["calls"]):
        for op in call["ops"]:
            if op[0] == "retune":
                n = len(op[2])
                inc[op[1]:op[1] + n], shift[op[1]:op[1] + n] = op[2], op[3]
            elif op[0] == "move":
                src[op[1]] = op[2]
            elif op[0] == "reset":
                epoch0 = at
            else:
                device = not device
        nb = call["units"] * unit
        yield (i, device, call["ops"], cfg["wide"][:, epoch0:at + nb], (at - epoch0) // (2 * M), nb // (2 * M),
               src.copy(), inc.copy(), shift.copy())
        at += nb


def first_channel_kills(cfg, P):
    """The mutants of tests/chan_mutants.py that channel 0 of this case exposes (CPU only)."""
    killed = set()
    for _, _, _, epoch, m0, n_out, src, inc, shift in walk(cfg):
        out = mu.all_outputs(epoch[src[0]], cfg["h"], cfg["M"], int(inc[0]), int(shift[0]), P, m_range=(m0, m0 + n_out))
        killed |= {m for m in mu.MUTANTS if not np.array_equal(out[m], out[None])}
    return killed


class Context:
    """The pieces every case shares: the library, its phasor table, one engine for the plain cases."""

    def __init__(self, oracle=None):
        self.capi, self.P, self.oracle = capi, capi.channelizer_phasor_table(), oracle
        self.eng = capi.Engine(1)
        self.stats = {}            # what the scan cases met (blocks of checked following channels): see run_scan

    def count(self, key, n=1):
        self.stats[key] = self.stats.get(key, 0) + int(n)

    def close(self):
        self.eng.close()


def run_plain(cfg, ctx, before_call=None):
    """Runs the case's script through iqd_channelizer_run / run_device; None, or what differed.  before_call(z, i, device,
    piece, epoch, m0, n_out): a step before call i (a survey case's), returning None or what differed."""
    eng, P, M = ctx.eng, ctx.P, cfg["M"]
    z = capi.Channelizer(eng, M, cfg["n_ch"], n_sources=cfg["n_src"], taps=cfg["taps"])
    z.set_channels(0, source=cfg["src"], phase_inc=cfg["inc"], gain_shift=cfg["shift"])
    bad = None
    for i, device, ops, epoch, m0, n_out, src, inc, shift in walk(cfg):
        for op in ops:
            if op[0] == "retune":
                z.set_channels(op[1], phase_inc=op[2], gain_shift=op[3])
            elif op[0] == "move":
                z.set_channels(op[1], source=[op[2]])
            elif op[0] == "reset":
                z.reset()
        piece = np.ascontiguousarray(epoch[:, 2 * M * m0:])
        if before_call:
            bad = before_call(z, i, device, piece, epoch, m0, n_out)
            if bad:
                break
        if device:
            d_in, d_out = eng.dev_alloc(piece.nbytes), eng.dev_alloc(cfg["n_ch"] * 2 * n_out)
            eng.dev_upload(d_in, piece)
            z.run_device(d_in, piece.shape[1], d_out)
            eng.synchronize()
            got = eng.dev_download(d_out, cfg["n_ch"] * 2 * n_out).reshape(cfg["n_ch"], -1)
            eng.dev_free(d_in)
            eng.dev_free(d_out)
        else:
            got = z.run(piece)
        for c in cfg["check"]:
            want = cm.channel(epoch[src[c]], cfg["h"], M, int(inc[c]), int(shift[c]), P, m_range=(m0, m0 + n_out))
            if not np.array_equal(got[c], want):
                d = np.flatnonzero(got[c] != want)
                bad = ("call %d (%s form, %d outputs from output %d of the epoch): channel %d (source %d inc 0x%08x L %d) "
                       "differs in %d bytes, first at byte %d (outputs %s): got %s, model %s" % (
                           i, "device" if device else "host", n_out, m0, c, src[c], inc[c], shift[c], len(d), d[0],
                           np.unique(d // 2)[:12].tolist(), got[c][d[:8]].tolist(), want[d[:8]].tolist()))
                break
        if bad:
            break
    z.close()
    return bad


def plain_case(rng, ctx):
    cfg = draw_plain(rng)
    bad = run_plain(cfg, ctx)
    return None if bad is None else "plain case: %s\n  %s" % (describe(cfg), bad)


# ------------------------------------------------------------------------------------------------ fractional cases
def frac_t_max(P, Q, kb):
    """outputs per window of chz_frac_kernel (iqd_chan.cpp: chz_launch)"""
    kp = (kb + 31) // 32 * 32
    g = 16 * max(4, Q)
    return min(1024, (12288 - kp) * Q // P) // g * g


def draw_frac(rng):
    """One fractional case, drawn without a GPU: decimation P / Q with gcd(P, Q) = 1 and 2 <= P / Q <= 64, a prototype of
    up to 1024 Q taps within the per-branch bound (or the default one), calls in units of 64 P bytes with the operator
    steps of the plain cases between them."""
    Q = int(rng.choice([2, 4, 8]))
    hi = 64 * Q if rng.random() < 0.25 else 12 * Q          # mostly modest ratios: the model's cost grows with P
    P = int(rng.integers(Q, hi // 2)) * 2 + 1
    r = rng.random()
    if r < 0.35:
        taps, h = None, capi.channelizer_default_taps(P, Q)
    else:
        K = int(rng.choice([1, Q - 1, Q, Q + 1, 32 * Q - 1, 32 * Q + 1, 1024 * Q - int(rng.integers(0, Q))])) if r < 0.6 \
            else int(rng.integers(1, 1024 * Q + 1))
        kb = -(-K // Q)
        smax = min(32639, BOUND_SUM // kb)
        sc = smax if rng.random() < 0.2 else int(2.0 ** rng.uniform(3, np.log2(smax)))
        taps = h = rng.integers(-sc, sc + 1, K).astype(np.int16)
    n_src = int(rng.integers(1, 4))
    n_ch = draw_count(rng)
    src = rng.integers(0, n_src, n_ch).astype(np.uint32)
    inc = np.array([draw_inc(rng) for _ in range(n_ch)], np.uint64)
    shift = rng.integers(0, 9, n_ch).astype(np.uint8)
    tm = frac_t_max(P, Q, -(-len(h) // Q))
    calls = []
    for i in range(int(rng.integers(1, 7))):
        u = 1 if rng.random() < 0.4 else int(rng.integers(2, 7))
        if rng.random() < 0.15 and not any(c["units"] > 8 for c in calls):
            u = tm // (32 * Q) + int(rng.integers(1, 4))    # several windows
        ops = []
        if calls and rng.random() < 0.5:
            what = int(rng.integers(0, 4))
            if what == 0:
                first = int(rng.integers(0, n_ch))
                n = int(rng.integers(1, min(4, n_ch - first) + 1))
                ops.append(("retune", first, [draw_inc(rng) for _ in range(n)], [int(v) for v in rng.integers(0, 9, n)]))
            elif what == 1:
                ops.append(("move", int(rng.integers(0, n_ch)), int(rng.integers(0, n_src))))
            elif what == 2:
                ops.append(("reset",))
            else:
                ops.append(("form",))
        calls.append({"units": u, "ops": ops})
    total = sum(c["units"] for c in calls) * 32 * P
    kinds, wide = [], []
    for s in range(n_src):
        k, w = draw_input(rng, -(-P // Q), total)
        kinds.append(k)
        wide.append(w)
    work = 4.0 * -(-len(h) // Q) * sum(c["units"] for c in calls) * 32 * Q
    n_check = int(max(min(4, n_ch), min(n_ch if n_ch <= 64 else 32, MODEL_BUDGET // work)))
    check = np.arange(n_ch) if n_check >= n_ch else np.unique(np.concatenate(
        [[0, n_ch - 1], rng.choice(n_ch, n_check, replace=False)]))
    return {"M": P, "Q": Q, "K": len(h), "taps": taps, "h": h, "n_src": n_src, "n_ch": n_ch, "src": src, "inc": inc,
            "shift": shift, "calls": calls, "kinds": kinds, "wide": np.stack(wide), "check": check,
            "device_form": bool(rng.random() < 0.5)}


def run_frac(cfg, ctx, before_call=None):
    """Runs a fractional case's script through iqd_channelizer_run / run_device; None, or what differed (before_call: as
    in run_plain)."""
    eng, Pt, P, Q = ctx.eng, ctx.P, cfg["M"], cfg["Q"]
    z = capi.Channelizer(eng, P, cfg["n_ch"], n_sources=cfg["n_src"], taps=cfg["taps"], decimation_den=Q)
    z.set_channels(0, source=cfg["src"], phase_inc=cfg["inc"], gain_shift=cfg["shift"])
    bad = None
    # walk() counts a call's outputs as for an integer decimation by P: Q times as many here
    for i, device, ops, epoch, t0, nt, src, inc, shift in walk(cfg):
        m0, n_out = t0 * Q, nt * Q
        for op in ops:
            if op[0] == "retune":
                z.set_channels(op[1], phase_inc=op[2], gain_shift=op[3])
            elif op[0] == "move":
                z.set_channels(op[1], source=[op[2]])
            elif op[0] == "reset":
                z.reset()
        piece = np.ascontiguousarray(epoch[:, 2 * P * t0:])
        if before_call:
            bad = before_call(z, i, device, piece, epoch, m0, n_out)
            if bad:
                break
        if device:
            d_in, d_out = eng.dev_alloc(piece.nbytes), eng.dev_alloc(cfg["n_ch"] * 2 * n_out)
            eng.dev_upload(d_in, piece)
            z.run_device(d_in, piece.shape[1], d_out)
            eng.synchronize()
            got = eng.dev_download(d_out, cfg["n_ch"] * 2 * n_out).reshape(cfg["n_ch"], -1)
            eng.dev_free(d_in)
            eng.dev_free(d_out)
        else:
            got = z.run(piece)
        ck = cfg["check"]
        want = fm.channelize(epoch, cfg["h"], P, Q, src[ck], inc[ck], shift[ck], Pt, m_range=(m0, m0 + n_out))
        for j, c in enumerate(ck):
            if not np.array_equal(got[c], want[j]):
                d = np.flatnonzero(got[c] != want[j])
                bad = ("call %d (%s form, %d outputs from output %d of the epoch): channel %d (source %d inc 0x%08x L %d) "
                       "differs in %d bytes, first at byte %d (outputs %s): got %s, model %s" % (
                           i, "device" if device else "host", n_out, m0, c, src[c], inc[c], shift[c], len(d), d[0],
                           np.unique(d // 2)[:12].tolist(), got[c][d[:8]].tolist(), want[j][d[:8]].tolist()))
                break
        if bad:
            break
    z.close()
    return bad


def frac_case(rng, ctx):
    cfg = draw_frac(rng)
    bad = run_frac(cfg, ctx)
    return None if bad is None else "fractional case (decimation %d/%d): %s\n  %s" % (cfg["M"], cfg["Q"], describe(cfg), bad)


# ---------------------------------------------------------------------------------------------------- survey cases
def survey_case(rng, ctx):
    """A plain or a fractional case (drawn as ever) with survey steps between its calls: the points are set before the
    first call - now and then again, or cleared and set again, later - and before about two calls in three the call's
    bytes are surveyed first, in the form the call takes, at a block size drawn from the admissible ones."""
    frac = rng.random() < 0.35
    cfg = draw_frac(rng) if frac else draw_plain(rng)
    M, Q, h, n_src = cfg["M"], cfg.get("Q", 1), cfg["h"], cfg["n_src"]
    units = sum(c["units"] for c in cfg["calls"])
    work = 4.0 * -(-len(h) // Q) * (M if Q == 1 else Q) * units * 32 * n_src      # the model's cost per point
    n_pts = int(min(int(rng.choice([1, 7, 8, 9, 17, 65])), max(1, MODEL_BUDGET // work)))
    draw_pts = lambda: ([draw_inc(rng) for _ in range(n_pts)], [int(v) for v in rng.integers(0, 9, n_pts)])   # noqa: E731
    pts = [draw_pts()]
    steps = []
    for i, call in enumerate(cfg["calls"]):
        n_out = call["units"] * 32 * Q
        step = 128 if Q > 1 else 32
        sizes = [b for b in range(step, n_out + 1, step) if n_out % b == 0]
        new = i > 0 and rng.random() < 0.2
        if new:
            pts.append(draw_pts())
        steps.append({"points": len(pts) - 1 if new or i == 0 else None, "clear_first": bool(new and rng.random() < 0.5),
                      "block_out": int(rng.choice(sizes)) if sizes and rng.random() < 0.67 else 0})
    state = {}
    win = frac_t_max(M, Q, -(-len(h) // Q)) if Q > 1 else t_max(M, len(h))

    def before_call(z, i, device, piece, epoch, m0, n_out):
        st = steps[i]
        if st["points"] is not None:
            if st["clear_first"]:
                z.set_survey(phase_inc=[])
            state["inc"], state["shift"] = pts[st["points"]]
            z.set_survey(phase_inc=state["inc"], gain_shift=state["shift"])
        if not st["block_out"]:
            return None
        bo = st["block_out"]
        want = svm.survey(epoch, h, M, Q, state["inc"], state["shift"], ctx.P, bo, m0, n_out, win, ctx.oracle)
        if device:
            d_in, d_mag = ctx.eng.dev_alloc(piece.nbytes), ctx.eng.dev_alloc(want.nbytes)
            ctx.eng.dev_upload(d_in, piece)
            z.survey_device(d_in, piece.shape[1], 2 * bo, d_mag)
            ctx.eng.synchronize()
            got = ctx.eng.dev_download(d_mag, want.nbytes, np.uint32).reshape(want.shape)
            ctx.eng.dev_free(d_in)
            ctx.eng.dev_free(d_mag)
        else:
            got = z.survey(piece, 2 * bo)
        ctx.count("surveys")
        ctx.count("survey blocks", want.shape[1])
        if np.array_equal(got, want):
            return None
        d = np.argwhere(got != want)
        return ("survey before call %d (%s form, %d outputs from output %d of the epoch, blocks of %d outputs, %d points): %d "
                "entries differ, first (source, block, point) %s: got %d, model %d; inc %r shift %r" % (
                    i, "device" if device else "host", n_out, m0, bo, n_pts, len(d), d[0].tolist(), got[tuple(d[0])],
                    want[tuple(d[0])], state["inc"][:16], state["shift"][:16]))

    bad = (run_frac if frac else run_plain)(cfg, ctx, before_call)
    return None if bad is None else "survey case (decimation %d/%d; survey steps %r): %s\n  %s" % (M, Q, steps, describe(cfg), bad)


# ------------------------------------------------------------------------------------------------------ scan cases
BASE_HZ = 1_700_000_000


def _dev_call(eng, z, wide, bb, first=0):
    """iqd_accept_wideband_device -> rows, pcm, counts, magnitude, allowed"""
    n, bps = z.n_channels, wide.shape[1]
    row = bps // z.decimation
    nblk = row // bb if row % bb == 0 else 1
    sizes = (wide.nbytes, n * row, n * row // 64 * 2, 4 * n, 4 * n * nblk, n * nblk)
    d = [eng.dev_alloc(max(16, s)) for s in sizes]
    eng.dev_upload(d[0], np.ascontiguousarray(wide))
    eng.accept_wideband_device(z, d[0], bps, d[1], d[2], d[3], d[4], d[5], first=first)
    eng.synchronize()
    out = (eng.dev_download(d[1], n * row).reshape(n, row), eng.dev_download(d[2], n * row // 64 * 2, np.int16).reshape(n, -1),
           eng.dev_download(d[3], 4 * n, np.uint32), eng.dev_download(d[4], 4 * n * nblk, np.uint32).reshape(n, nblk),
           eng.dev_download(d[5], n * nblk).reshape(n, nblk))
    for p in d:
        eng.dev_free(p)
    return out


def draw_grid(rng, M, centre, rot):
    """A scan grid in station Hz around one source: inside the band, leaving it on either side, or touching the offsets
    o = -Fs/2, Fs/2 - 1 and Fs/2 exactly (o = station + 64000 rot - centre)."""
    fs = 256000 * M
    st0 = centre - 64000 * rot                  # the station whose offset is 0
    kind = int(rng.integers(0, 5))
    step = int(rng.choice([fs // 16, fs // 8, 12500, fs // 4]))
    if kind == 0:
        start = st0 + int(rng.integers(-fs // 2, fs // 4))
        return start, start + step * int(rng.integers(1, 6)), step
    if kind == 1:                               # leaves the band at the top
        start = st0 + fs // 2 - step * int(rng.integers(1, 4))
        return start, start + step * 6, step
    if kind == 2:                               # starts below the band
        start = st0 - fs // 2 - step * int(rng.integers(1, 4))
        return start, start + step * 6, step
    if kind == 3:                               # ends exactly on o = Fs/2 (out), the step before on Fs/2 - 1 (in)
        return st0 + fs // 2 - 3, st0 + fs // 2, 1
    return st0 - fs // 2 - step, st0 - fs // 2 + step, step      # passes o = -Fs/2 exactly (in band)


def run_scan(ctx, M, taps, h, n_src, n_ch, bb, calls, rng, check=None, follow_p=0.75, what="scan case"):
    """Following and fixed channels through iqd_accept_wideband_device, against chan_scan_model.follow on oracle chains.
    calls: engine blocks per call (0: one short block).  None, or what differed."""
    P = ctx.P
    fs, bo = 256000 * M, bb // 2
    centres = [BASE_HZ + 3_000_000 * s + int(rng.integers(0, 1000)) for s in range(n_src)]
    src = rng.integers(0, n_src, n_ch).astype(np.uint32)
    inc = np.array([draw_inc(rng) for _ in range(n_ch)], np.uint64)
    shift = rng.integers(0, 4, n_ch).astype(np.uint8)
    follow = rng.random(n_ch) < follow_p
    follow[0] = True
    outs = [k * bo if k else 32 * int(rng.integers(1, max(2, bo // 32))) for k in calls]
    total = sum(outs)
    stations = lambda s: [{"offset": int(f * fs), "kind": ("fm", "am")[i % 2], "amplitude": 40.0,   # noqa: E731
                           "on": [(int(a), int(a) + int(rng.integers(bo * M, 3 * bo * M + 1)))
                                  for a in rng.integers(0, max(1, total * M), 2)]}
                          for i, f in enumerate((-0.3, -0.1, 0.15, 0.35))]
    wide = np.stack([synth.wideband(total * M, fs, stations(s), seed=int(rng.integers(1 << 30)), sigma=1.0)
                     for s in range(n_src)])
    check = list(range(n_ch)) if check is None else check
    eng = capi.Engine(n_ch, block_bytes=bb)
    eng.set_gain_trace(True)
    chains = {c: ctx.oracle.chain() for c in check}
    setup = []
    for c in range(n_ch):
        rot = int(rng.integers(-1, 2))
        th = int(rng.choice([-200, -60, -50, -45, 0]))
        agc = int(rng.integers(0, 2)) if rng.random() < 0.3 else None
        grid = draw_grid(rng, M, centres[src[c]], rot)
        setup.append([rot, th, agc, grid])
        eng.set_mode("fm", c, 1)
        eng.set_squelch(th, c, 1)
        eng.set_rotation(rot, c, 1)
        eng.scanner_set_parameters(*grid, first=c, n=1)
        eng.scanner_start(True, c, 1)
        if agc is not None:
            eng.agc_set_type(agc, c, 1)
            eng.agc_enable(True, c, 1)
        if c in chains:
            ch = chains[c]
            ch.set_mode("fm")
            ch.set_squelch(th)
            ch.set_rotation(rot)
            ch.scanner_set_parameters(*grid)
            ch.scanner_start()
            if agc is not None:
                ch.agc_set_type(agc)
                ch.agc_enable(True)
    z = capi.Channelizer(eng, M, n_ch, n_src, taps=taps)
    z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    z.set_source_frequency(centres)
    for c in np.flatnonzero(follow):
        z.follow_scanner(True, int(c), 1)
    log, bad, m_at = [], None, 0
    for i, n_out in enumerate(outs):
        if i and rng.random() < 0.6:                       # between calls: follow toggled, or a scanner command
            c = int(rng.choice(check))
            op = int(rng.integers(0, 4))
            if op == 0:
                follow[c] = not follow[c]
                z.follow_scanner(bool(follow[c]), c, 1)
                log.append((i, c, "follow", bool(follow[c])))
                ctx.count("follow toggles")
            elif op == 1:
                eng.scanner_start(False, c, 1)
                chains[c].scanner_stop()
                log.append((i, c, "stop"))
                ctx.count("scanner commands")
            elif op == 2:                                  # (parameters are refused while scanning: stop first)
                grid = draw_grid(rng, M, centres[src[c]], setup[c][0])
                eng.scanner_start(False, c, 1)
                chains[c].scanner_stop()
                eng.scanner_set_parameters(*grid, first=c, n=1)
                eng.scanner_start(True, c, 1)
                chains[c].scanner_set_parameters(*grid)
                chains[c].scanner_start()
                log.append((i, c, "grid", grid))
                ctx.count("scanner commands")
            else:
                eng.scanner_start(True, c, 1)
                chains[c].scanner_start()
                log.append((i, c, "start"))
                ctx.count("scanner commands")
        nblk = calls[i] if calls[i] else 1
        blk = n_out // nblk
        piece = wide[:, 2 * M * m_at:2 * M * (m_at + n_out)]
        rows, pcm, cnt, mag, alw = _dev_call(eng, z, piece, bb)
        trace = eng.frequency_trace(nblk)
        for c in check:
            s = int(src[c])
            if follow[c]:
                f0 = sm.scanner_hz(chains[c])
                r, p, mg, al, tr = sm.follow(chains[c], wide[s], h, M, P, int(shift[c]), centres[s], blk, nblk,
                                             m_first=m_at, rotation=setup[c][0])
                quiet = (r.reshape(nblk, -1) == 0x80).all(axis=1)
                ctx.count("blocks", nblk)
                ctx.count("silent blocks", quiet.sum())
                ctx.count("open blocks", (al != 0).sum())
                ctx.count("closed blocks", (al == 0).sum())
                ctx.count("retunes", (np.concatenate([[f0], tr[:-1]]) != tr).sum())
                ctx.count("short blocks", calls[i] == 0)
                ctx.count("agc blocks", nblk if setup[c][2] is not None else 0)
            else:
                r = cm.channel(wide[s], h, M, int(inc[c]), int(shift[c]), P, m_range=(m_at, m_at + n_out))
                p, mg, al = chains[c].accept_stream(r, block_bytes=2 * blk)
                tr = None                                    # (its scanner runs on all the same: the chain steps with it)
            diff = ("rows" if not np.array_equal(rows[c], r) else
                    "pcm" if cnt[c] != len(p) or not np.array_equal(pcm[c, :cnt[c]], p) else
                    "magnitude" if not np.array_equal(mag[c], mg) else
                    "allowed" if not np.array_equal(alw[c], al) else
                    "frequency trace" if follow[c] and not np.array_equal(trace[c], tr) else None)
            if diff:
                d = np.flatnonzero(rows[c] != r)
                bad = ("%s: M=%d K=%d (%s) sources=%d channels=%d block_bytes=%d calls(outputs)=%r: call %d, channel %d "
                       "(source %d, following %s, rot/threshold/agc/grid %r, centre %d, L %d) differs in %s%s; ops %r" % (
                           what, M, len(h), "default taps" if taps is None else "given taps", n_src, n_ch, bb, outs, i, c,
                           s, bool(follow[c]), setup[c], centres[s], shift[c], diff,
                           " (%d bytes, first at %d)" % (len(d), d[0]) if len(d) else "", log))
                break
        if bad:
            break
        m_at += n_out
    z.close()
    eng.close()
    return bad


def scan_case(rng, ctx):
    M = int(rng.integers(2, 65))
    if rng.random() < 0.5:
        taps, h = None, capi.channelizer_default_taps(M)
    else:
        K = int(rng.choice(K_EDGES)) if rng.random() < 0.5 else int(rng.integers(1, 1025))
        taps = h = rng.integers(-4000, 4001, K).astype(np.int16)
    bb = int(rng.choice([256, 2048, 4096, 32768]))
    n_ch = int(rng.choice([1, 3, 8, 9, 17]))
    n_src = int(rng.integers(1, 4))
    budget = 6 * 4096 // 2                                  # outputs per case and channel
    per = max(1, min(5, budget // (bb // 2)))
    calls = [0 if rng.random() < 0.25 else int(rng.integers(1, per + 1)) for _ in range(int(rng.integers(1, 5)))]
    n_check = max(1, min(n_ch, int(MODEL_BUDGET // 2 // (4.0 * len(h) * M * max(32, sum(c * bb // 2 for c in calls))))))
    check = sorted(set([0] + rng.choice(n_ch, n_check, replace=False).tolist()))
    return run_scan(ctx, M, taps, h, n_src, n_ch, bb, calls, rng, check=check)


# ------------------------------------------------------------------------------------------------------ track cases
def track_case(rng, ctx):
    """Track-following and fixed channels of one channelizer against chan_track_model.Follower (fixed ones against
    chan_model): M, taps (K up to 1024: both kernel forms), sources, channels, S, block_bytes (64 ... 4096, no multiple of the
    window among them), blocks per call, lag, min_state and the call form drawn; a new synthetic table per call; between calls
    followers stop, start or move to another slot, and now and then the channelizer is reset.  Rows in the three forms that
    return them, PCM, magnitudes and flags against oracle chains in the two accept forms.  None, or what differed."""
    P = ctx.P
    M = int(rng.choice([2, 3, 7, 8, 16, 64])) if rng.random() < 0.7 else int(rng.integers(2, 65))
    taps, h = draw_taps(rng, M)
    K = len(h)
    n_src = int(rng.integers(1, 4))
    n_ch = min(draw_count(rng), 130)
    S = int(rng.choice([1, 2, 8, 64])) if rng.random() < 0.6 else int(rng.integers(1, 65))
    bb = 64 * int(rng.choice([1, 1, 2, 3, 4, 8, 16, 40, 64]))
    nblk = int(rng.integers(1, 7))
    while nblk * bb > 16384:
        nblk -= 1
    n_calls = int(rng.integers(2, 5))
    lag, min_state = int(rng.integers(0, 2)), int(rng.integers(1, 3))
    form = ("run", "run_device", "accept", "accept_device")[int(rng.integers(0, 4))]
    row = nblk * bb
    engine_bb = 256 if row % 256 == 0 else 32768               # whole engine blocks, or one short block
    src = rng.integers(0, n_src, n_ch).astype(np.uint32)
    inc = np.array([draw_inc(rng) for _ in range(n_ch)], np.uint64)
    shift = rng.integers(0, 9, n_ch).astype(np.uint8)
    slot = np.where(rng.random(n_ch) < 0.7, rng.integers(0, S, n_ch), -1).astype(np.int32)
    if not (slot >= 0).any():
        slot[0] = 0
    n_samp = n_calls * row // 2 * M
    wide = np.stack([draw_input(rng, M, n_samp)[1] for _ in range(n_src)])
    per = max(1, K * row // 2 * M * n_calls)
    check = sorted(rng.choice(n_ch, min(n_ch, max(2, int(MODEL_BUDGET // per))), replace=False).tolist())
    window = min(capi.channelizer_window_outputs(M, K), capi.channelizer_track_window_outputs(M, K))
    ctx.count("track cases")
    ctx.count("large K cases", K > 256)
    ctx.count("two-window cases", bb // 2 > window)
    eng = capi.Engine(n_ch, block_bytes=engine_bb)
    eng.set_mode("fm")
    eng.set_squelch(-45)
    z = capi.Channelizer(eng, M, n_ch, n_src, taps=taps)
    z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    z.follow_tracks(slot)
    fol = {c: tkm.Follower(h, M, P, src[c], shift[c], max(int(slot[c]), 0), channel=c, window=window) for c in check}
    chains = {}
    if form.startswith("accept"):
        for c in check:
            chains[c] = ctx.oracle.chain()
            chains[c].set_mode("fm")
            chains[c].set_squelch(-45)
    log, pos, bad, keep = [], 0, None, []
    span = row * M
    for i in range(n_calls):
        if i and rng.random() < 0.6:                           # between calls: stop, start or move a follower; or a reset
            if rng.random() < 0.25:
                z.reset()
                for f in fol.values():
                    f.reset()
                pos = 0
                log.append((i, "reset"))
                ctx.count("track resets")
            else:
                c = int(rng.integers(0, n_ch))
                new = -1 if slot[c] >= 0 and rng.random() < 0.5 else int(rng.integers(0, S))
                if new != slot[c]:
                    z.follow_tracks([new], first=c)
                    slot[c] = new
                    if c in fol and new >= 0:
                        fol[c].start(new)
                    log.append((i, c, "slot", new))
                    ctx.count("track toggles")
        table = tkc.synthetic_table(rng, n_src, nblk, S, nblk)
        d_t = eng.dev_alloc(table.nbytes)
        keep.append(d_t)
        eng.dev_upload(d_t, table.view(np.uint8).reshape(-1))
        if not (slot >= 0).any():                              # (every follower stopped: the call needs no table)
            z.set_track_table(None)
        else:
            z.set_track_table(d_t, S, nblk, bb, lag, min_state)
        piece = np.ascontiguousarray(wide[:, pos * span:(pos + 1) * span])
        rows = acc = None
        if form == "run":
            rows = z.run(piece)
        elif form == "accept":
            acc = eng.accept_wideband(z, piece)
        else:
            d_w, d_r = eng.dev_alloc(piece.nbytes), eng.dev_alloc(n_ch * row)
            eng.dev_upload(d_w, piece)
            if form == "run_device":
                z.run_device(d_w, span, d_r)
                eng.synchronize()
            else:
                nb_e = max(1, row // engine_bb)
                d_p, d_c, d_m, d_a = eng.dev_alloc(n_ch * row // 64 * 2), eng.dev_alloc(4 * n_ch), eng.dev_alloc(4 * n_ch * nb_e), eng.dev_alloc(n_ch * nb_e)
                eng.accept_wideband_device(z, d_w, span, d_r, d_p, d_c, d_m, d_a)
                eng.synchronize()
                acc = (eng.dev_download(d_p, n_ch * row // 64 * 2, np.int16).reshape(n_ch, -1), eng.dev_download(d_c, 4 * n_ch, np.uint32),
                       eng.dev_download(d_m, 4 * n_ch * nb_e, np.uint32).reshape(n_ch, nb_e), eng.dev_download(d_a, n_ch * nb_e).reshape(n_ch, nb_e))
                for d in (d_p, d_c, d_m, d_a):
                    eng.dev_free(d)
            rows = eng.dev_download(d_r, n_ch * row).reshape(n_ch, row)
            eng.dev_free(d_w)
            eng.dev_free(d_r)
        for c in check:
            wide_row = wide[src[c], :(pos + 1) * span]
            if slot[c] >= 0:
                want = fol[c].call(wide_row, table, bb, lag, min_state)
                live = (want.reshape(nblk, bb) != 0x80).any(axis=1)
                ctx.count("track blocks", nblk)
                ctx.count("live blocks", live.sum())
            else:
                m0 = pos * row // 2
                want = cm.channel(wide_row, h, M, int(inc[c]), int(shift[c]), P, m_range=(m0, m0 + row // 2))
                fol[c].skip(row // 2)
            what = None
            if rows is not None and not np.array_equal(rows[c], want):
                what = "rows (first at byte %d)" % int(np.nonzero(rows[c] != want)[0][0])
            if what is None and acc is not None:
                p_, mg, al = chains[c].accept_stream(want, block_bytes=min(engine_bb, len(want)))
                pcm, cnt, mag, alw = acc
                if cnt[c] != len(p_) or not np.array_equal(pcm[c, :cnt[c]], p_):
                    what = "pcm"
                elif not np.array_equal(mag[c], mg) or not np.array_equal(alw[c], al):
                    what = "magnitude / flags"
            if what is not None:
                bad = ("track case: M=%d K=%d (%s) sources=%d channels=%d S=%d block_bytes=%d blocks=%d lag=%d min_state=%d form=%s: "
                       "call %d, channel %d (source %d, slot %d, L %d) differs in %s; ops %r" % (
                           M, K, "default taps" if taps is None else "drawn taps", n_src, n_ch, S, bb, nblk, lag, min_state, form, i, c,
                           int(src[c]), int(slot[c]), int(shift[c]), what, log))
                break
        pos += 1
        if bad is not None:
            break
    for ch in chains.values():
        ch.close()
    z.close()
    for d in keep:
        eng.dev_free(d)
    eng.close()
    return bad


# ------------------------------------------------------------------------------------------------------ gain cases
def gain_case(rng, ctx):
    """Gain-following and fixed channels of one channelizer through iqd_accept_wideband_device, against
    chan_gain_model.follow on oracle chains: engine blocks of 256 ... 32768 bytes, per channel an AGC (either type, or
    off) with its operating point, deadband and blanking limit drawn, manual gains 0 ... 60 set between calls and the
    following flag toggled.  None, or what differed."""
    P = ctx.P
    M = int(rng.integers(2, 65))
    if rng.random() < 0.6:
        taps, h = None, capi.channelizer_default_taps(M)
    else:
        K = int(rng.choice(K_EDGES)) if rng.random() < 0.5 else int(rng.integers(1, 1025))
        hh = np.abs(np.sinc((np.arange(K) - (K - 1) / 2) / max(2.0, M)))
        taps = h = np.clip(np.rint(hh / hh.sum() * 32768 * rng.uniform(0.3, 1.0) * rng.choice([-1, 1], K)), -32639, 32639).astype(np.int16)
    cap = int(min(32768, max(128, 1e8 // (len(h) * M))))     # outputs per call the model can afford (it convolves at the wide rate)
    bb = int(rng.choice([b for b in (256, 1024, 2560, 4096, 32768) if b // 2 <= cap]))
    bo, fs = bb // 2, 256000 * M
    n_ch = int(rng.choice([1, 3, 8, 9, 17]))
    n_src = int(rng.integers(1, 4))
    per = max(1, min(6, cap // bo))
    calls = [0 if rng.random() < 0.25 else int(rng.integers(1, per + 1)) for _ in range(int(rng.integers(1, 5)))]
    outs = [k * bo if k else 32 * int(rng.integers(1, max(2, bo // 32))) for k in calls]
    total = sum(outs)
    n_check = max(1, min(n_ch, int(MODEL_BUDGET // 2 // (4.0 * len(h) * M * max(32, total)))))
    check = sorted(set([0] + rng.choice(n_ch, n_check, replace=False).tolist()))
    src = rng.integers(0, n_src, n_ch).astype(np.uint32)
    fracs = rng.uniform(-0.45, 0.45, 4)
    stations = [{"offset": float(f) * fs, "kind": "fm", "amplitude": float(2.0 ** rng.uniform(0, 6.3))} for f in fracs[:3]]
    wide = np.stack([synth.wideband(total * M, fs, stations, seed=int(rng.integers(1 << 30)), sigma=float(rng.choice([0.3, 1.0, 4.0])))
                     if rng.random() < 0.8 else draw_input(rng, M, total * M)[1] for _ in range(n_src)])
    inc = np.array([capi.phase_inc(float(rng.choice(fracs)) * fs, fs) if rng.random() < 0.7 else draw_inc(rng) for _ in range(n_ch)],
                   np.uint64)
    shift = rng.integers(0, 9, n_ch).astype(np.uint8)
    follow = rng.random(n_ch) < 0.75
    follow[0] = True
    eng = capi.Engine(n_ch, block_bytes=bb)
    eng.set_gain_trace(True)
    chains = {c: ctx.oracle.chain() for c in check}
    setup = []
    for c in range(n_ch):
        th = int(rng.choice([-200, -60, -45, -30]))
        agc = int(rng.integers(0, 2)) if rng.random() < 0.7 else None
        op, dead, blank = int(rng.integers(-24, -3)), int(rng.integers(0, 4)), int(rng.integers(0, 4))
        g0 = int(rng.integers(0, 61 if agc is None else 47))   # (a running AGC holds the gain within 0 ... 46)
        setup.append([th, agc, op, dead, blank, g0])
        for t in [eng] + ([chains[c]] if c in chains else []):
            a = (c, 1) if t is eng else ()
            t.set_mode("fm", *a)
            t.set_squelch(th, *a)
            t.set_rx_gain_db(g0, *a)
            t.agc_set_operating_point(op, *a)
            t.agc_set_deadband(dead, *a)
            t.agc_set_blanking_limit(blank, *a)
            if agc is not None:
                t.agc_set_type(agc, *a)
                t.agc_enable(True, *a)
    z = capi.Channelizer(eng, M, n_ch, n_src, taps=taps)
    z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    for c in np.flatnonzero(follow):
        z.follow_gain(True, int(c), 1)
    log, bad, m_at = [], None, 0
    for i, n_out in enumerate(outs):
        if i and rng.random() < 0.7:                       # between calls: follow toggled, or the operator's gain
            c = int(rng.choice(check))
            if rng.random() < 0.4:
                follow[c] = not follow[c]
                z.follow_gain(bool(follow[c]), c, 1)
                log.append((i, c, "follow", bool(follow[c])))
                ctx.count("follow toggles")
            else:
                g = int(rng.integers(0, 61 if setup[c][1] is None else 47))
                eng.set_rx_gain_db(g, c, 1)
                chains[c].set_rx_gain_db(g)
                log.append((i, c, "gain", g))
                ctx.count("manual gains")
        nblk = calls[i] if calls[i] else 1
        blk = n_out // nblk
        piece = wide[:, 2 * M * m_at:2 * M * (m_at + n_out)]
        rows, pcm, cnt, mag, alw = _dev_call(eng, z, piece, bb)
        trace = eng.gain_trace(nblk)
        for c in check:
            s = int(src[c])
            if follow[c]:
                r, p, mg, al, tr = gm.follow(chains[c], wide[s], h, M, int(inc[c]), P, blk, nblk, m_first=m_at)
                ctx.count("gain blocks", nblk)
                ctx.count("gain changes", (np.diff(tr.astype(np.int64)) != 0).sum())
                ctx.count("blocks above 46 dB", (tr > 46).sum())
                ctx.count("short blocks", calls[i] == 0)
            else:
                tr = []
                r = cm.channel(wide[s], h, M, int(inc[c]), int(shift[c]), P, m_range=(m_at, m_at + n_out))
                p, mg, al = [], [], []
                for b in range(nblk):                        # (block by block: the gain before each block is the trace's)
                    tr.append(chains[c].rx_gain_db())
                    pb, mb, ab = chains[c].accept_stream(r[2 * blk * b:2 * blk * (b + 1)], block_bytes=2 * blk)
                    p.append(pb); mg.append(mb[0]); al.append(ab[0])
                p, mg, al, tr = np.concatenate(p), np.array(mg), np.array(al), np.array(tr)
            diff = ("rows" if not np.array_equal(rows[c], r) else
                    "pcm" if cnt[c] != len(p) or not np.array_equal(pcm[c, :cnt[c]], p) else
                    "magnitude" if not np.array_equal(mag[c], mg) else
                    "allowed" if not np.array_equal(alw[c], al) else
                    "gain trace" if not np.array_equal(trace[c], tr) else None)
            if diff:
                d = np.flatnonzero(rows[c] != r)
                bad = ("gain case: M=%d K=%d (%s) sources=%d channels=%d block_bytes=%d calls(outputs)=%r: call %d, channel %d "
                       "(source %d, following %s, threshold/agc/operating point/deadband/blanking/gain %r, inc 0x%08x, L %d) "
                       "differs in %s%s; gains got %r model %r; ops %r" % (
                           M, len(h), "default taps" if taps is None else "given taps", n_src, n_ch, bb, outs, i, c, s,
                           bool(follow[c]), setup[c], inc[c], shift[c], diff,
                           " (%d bytes, first at %d)" % (len(d), d[0]) if len(d) else "", trace[c].tolist(),
                           np.asarray(tr).tolist(), log))
                break
        if bad:
            break
        m_at += n_out
    z.close()
    eng.close()
    return bad


# ---------------------------------------------------------------------------------------------------- format cases
# of the format cases: on the taps' limit with matched input; with a planted half point; draw_taps' taps at the bound
FMT_LIMIT_SHARE, FMT_PLANT_SHARE, FMT_BOUND_SHARE = 0.12, 0.25, 0.08
LIMIT_INCS = (0, 2 ** 29, 3 * 2 ** 29, 5 * 2 ** 29, 7 * 2 ** 29)   # 0 degrees and the diagonals (chan_fmt_cases.limit_taps)
LIMIT_SEG = 2048                                         # samples of one (rail, extreme) segment: twice the taps' reach


def draw_fmt_input(rng, fmt, M, n_samples):
    """(kind, [2 n_samples] of the format's dtype, the offset-binary capture it was converted from or None)"""
    kind = int(rng.integers(0, 5))
    r = np.random.default_rng(int(rng.integers(1 << 30)))
    dt = sfm.DTYPE[fmt]
    info = np.iinfo(dt)
    if kind == 0:
        return "full", fc.full_random(r, n_samples, fmt), None
    if kind == 1:                                             # (S16: the high byte is 0 or -1, the low one carries it all)
        return "small", fc.small_random(r, n_samples, fmt), None
    if kind == 2:
        return "rails", r.choice([info.min, info.max], 2 * n_samples).astype(dt), None
    if kind == 3:
        fs = 256000.0 * M
        st = [{"offset": float(rng.uniform(-0.45, 0.45)) * fs, "kind": ("fm", "am", "usb")[i % 3],
               "amplitude": float(2.0 ** rng.uniform(1, 5.5)), "tone": 1000.0 + 300 * i,
               "on": [(int(a), int(a) + int(rng.integers(1, n_samples + 1)))
                      for a in rng.integers(0, n_samples, 2)]} for i in range(int(rng.integers(1, 4)))]
        u8 = synth.wideband(n_samples, fs, st, seed=int(rng.integers(1 << 30)), sigma=float(rng.choice([0.0, 1.0, 4.0])))
        return "carriers", sfm.from_u8(u8, fmt).copy(), u8
    return "constant", np.tile(rng.integers(info.min, info.max + 1, 2).astype(dt), n_samples), None


def limit_input(h, M, inc, P, fmt, n_samples):
    """Rail input sign-matched to the taps of increment inc (chan_fmt_cases.limit_case's, at any M that is a multiple of
    the taps' period 8): segments of LIMIT_SEG samples for (rail, extreme) = (re, max), (re, min), (im, max), (im, min),
    over and over.  In the second half of a segment |A| is the largest the taps allow."""
    assert M % 8 == 0
    gr, gi = cm.channel_taps(h, inc, P)
    nn = np.arange(n_samples)
    k = (M - 1 - nn) % 8                                      # x[n] meets g[k], k = (n_m - n) mod 8, n_m = M - 1 mod 8
    sr = np.array([np.sign(gr[kk::8].sum()) for kk in range(8)])[k]
    si = np.array([np.sign(gi[kk::8].sum()) for kk in range(8)])[k]
    q = nn // LIMIT_SEG % 4
    wr, wi = np.where(q < 2, sr, si), np.where(q < 2, -si, sr)    # Ar = sum gr xr - gi xi, Ai = sum gr xi + gi xr
    wr, wi = np.where(q % 2 == 0, wr, -wr), np.where(q % 2 == 0, wi, -wi)
    info = np.iinfo(sfm.DTYPE[fmt])
    w = np.empty(2 * n_samples, sfm.DTYPE[fmt])
    w[0::2], w[1::2] = np.where(wr > 0, info.max, info.min), np.where(wi > 0, info.max, info.min)
    return w


def draw_fmt(rng):
    """One format case, drawn without a GPU: draw_plain's configuration and script on a signed capture.  cfg["wide"] is
    [n_src, 2 samples] of the format's dtype, so that walk() serves as it is (a unit is 64 M elements: 32 outputs)."""
    fmt = ("s8", "s16")[int(rng.integers(0, 2))]
    share = rng.random()
    limit = share < FMT_LIMIT_SHARE
    plant = not limit and share < FMT_LIMIT_SHARE + FMT_PLANT_SHARE
    bound = FMT_LIMIT_SHARE + FMT_PLANT_SHARE <= share < FMT_LIMIT_SHARE + FMT_PLANT_SHARE + FMT_BOUND_SHARE
    M = 8 * int(rng.integers(1, 9)) if limit else int(rng.choice([2, 64])) if rng.random() < 0.1 else int(rng.integers(2, 65))
    taps, h = draw_taps(rng, M)
    while bound and np.abs(h.astype(np.int64)).sum() != BOUND_SUM:      # draw_taps' own, until it is one of those
        taps, h = draw_taps(rng, M)
    if limit:
        taps = h = fc.limit_taps()
    elif plant and taps is not None and np.abs(h.astype(np.int64)).max() > 31:
        # small taps: the sample that plant_half changes may take any value, and the output byte must not saturate on it
        taps = h = (h.astype(np.int64) * 31 // np.abs(h.astype(np.int64)).max()).astype(np.int16)
    K = len(h)
    n_src = int(rng.integers(1, 5))
    used = [s for s in range(n_src) if rng.random() < 0.7] or [int(rng.integers(0, n_src))]   # the rest: no channel
    n_ch = draw_count(rng)
    src = rng.choice(used, n_ch).astype(np.uint32)
    inc = np.array([draw_inc(rng) for _ in range(n_ch)], np.uint64)
    shift = rng.integers(0, 9, n_ch).astype(np.uint8)
    src_inc = [int(rng.choice(LIMIT_INCS)) for _ in range(n_src)]       # limit cases: what a source's input is matched to
    if limit:
        for c in range(n_ch):
            if c == 0 or rng.random() < 0.5:
                inc[c] = src_inc[src[c]]
    if plant:
        inc[0], shift[0] = 0, 8              # real taps; L = 8: one LSB of stage a is two of the output byte
    win = capi.channelizer_window_outputs(M, K, fmt)
    calls, long_calls = [], 0
    for _ in range(int(rng.integers(1, 9))):
        r = rng.random()
        if r < 0.3:
            u = 1                                                       # the shortest call: 32 outputs
        elif r < 0.55:
            u = 2 * int(rng.integers(1, 6)) + 1                         # n_out % 64 == 32
        elif r < 0.8 or long_calls >= 2:
            u = 2 * int(rng.integers(1, 6))
        else:                                                           # several windows and a tail of 32, 96 or 160 outputs
            u = win // 32 * (2 if 2 * win <= 768 and rng.random() < 0.4 else 1) + 2 * int(rng.integers(0, 3)) + 1
            long_calls += 1
        ops = []
        if calls and rng.random() < 0.5:
            what = int(rng.integers(0, 4))
            if what == 0:
                first = int(rng.integers(0, n_ch))
                n = int(rng.integers(1, min(4, n_ch - first) + 1))
                ops.append(("retune", first, [draw_inc(rng) for _ in range(n)], [int(v) for v in rng.integers(0, 9, n)]))
            elif what == 1:
                ops.append(("move", int(rng.integers(0, n_ch)), int(rng.integers(0, n_src))))
            elif what == 2:
                ops.append(("reset",))
            else:
                ops.append(("form",))
        calls.append({"units": u, "ops": ops})
    if limit:                                # every segment once: the first call grows to what is missing
        calls[0]["units"] += max(0, -(-4 * LIMIT_SEG // (32 * M)) - sum(c["units"] for c in calls))
    units = sum(c["units"] for c in calls)
    total = units * 32 * M
    kinds, wide, u8 = [], [], {}
    for s in range(n_src):
        k, w, u = draw_fmt_input(rng, fmt, M, total)
        if limit:
            k, w, u = "limit 0x%08x" % src_inc[s], limit_input(h, M, src_inc[s], ctx_phasor(), fmt, total), None
        elif plant and s == src[0]:
            k, w, u = "small", fc.small_random(np.random.default_rng(int(rng.integers(1 << 30))), total, fmt), None
        kinds.append(k)
        wide.append(w)
        if u is not None:
            u8[s] = u
    # the channels compared: the first and the last, those an operator's step touches, and random ones within the budget
    # (the model gathers [outputs, K] per rail and call and multiplies it by the checked channels' taps)
    touched = [c for call in calls for op in call["ops"] if op[0] in ("retune", "move")
               for c in ([op[1], op[1] + len(op[2]) - 1] if op[0] == "retune" else [op[1]])]
    work = 4.0 * K * units * 32
    n_check = int(max(min(4, n_ch), min(n_ch if n_ch <= 64 else 32, MODEL_BUDGET // work)))
    check = np.arange(n_ch) if n_check >= n_ch else np.unique(np.concatenate(
        [[0, n_ch - 1], touched, rng.choice(n_ch, n_check, replace=False)]).astype(np.int64))
    cfg = {"fmt": fmt, "M": M, "K": K, "taps": taps, "h": h, "n_src": n_src, "n_ch": n_ch, "src": src, "inc": inc,
           "shift": shift, "calls": calls, "kinds": kinds, "wide": np.stack(wide), "u8": u8, "check": check,
           "device_form": bool(rng.random() < 0.5), "limit": limit, "window": win, "planted": None}
    if plant:                                # in a call that still finds channel 0 as it was set up, on the source it has then
        ok = [(epoch, m0, n_out, int(s_[0])) for _, _, _, epoch, m0, n_out, s_, i_, l_ in walk(cfg) if i_[0] == 0 and l_[0] == 8]
        epoch, m0, n_out, s0 = ok[int(rng.integers(0, len(ok)))]
        m_star = m0 + int(rng.integers(0, n_out))
        try:                                 # (epoch is a view of cfg["wide"]: from the last reset, which zeroed the history)
            fc.plant_half(epoch[s0], h, M, ctx_phasor(), m_star)
            cfg["planted"] = (s0, m_star)
        except AssertionError:               # (taps without an odd one: no sample value need do it)
            pass
    return cfg


_PHASOR = []


def ctx_phasor():
    if not _PHASOR:
        _PHASOR.append(capi.channelizer_phasor_table())
    return _PHASOR[0]


def describe_fmt(cfg):
    return "%s%s%s %s" % (cfg["fmt"], ", taps on the limit and matched rail input" if cfg["limit"] else "",
                          ", half point planted at (source, output of its epoch) %r" % (cfg["planted"],) if cfg["planted"] else "",
                          describe(cfg))


def run_fmt(cfg, ctx):
    """Runs a format case's script through iqd_channelizer_run / run_device of a channelizer of its sample format, every
    checked channel of every call against chan_fmt_model.channelize over the epoch; None, or what differed."""
    eng, P, M, fmt = ctx.eng, ctx.P, cfg["M"], cfg["fmt"]
    B = sfm.RAIL_BYTES[fmt]
    z = capi.Channelizer(eng, M, cfg["n_ch"], n_sources=cfg["n_src"], taps=cfg["taps"], sample_format=fmt)
    z.set_channels(0, source=cfg["src"], phase_inc=cfg["inc"], gain_shift=cfg["shift"])
    bad = None
    ck = cfg["check"]
    for i, device, ops, epoch, m0, n_out, src, inc, shift in walk(cfg):
        for op in ops:
            if op[0] == "retune":
                z.set_channels(op[1], phase_inc=op[2], gain_shift=op[3])
            elif op[0] == "move":
                z.set_channels(op[1], source=[op[2]])
            elif op[0] == "reset":
                z.reset()
        piece = np.ascontiguousarray(epoch[:, 2 * M * m0:])
        if device:
            d_in, d_out = eng.dev_alloc(piece.nbytes), eng.dev_alloc(cfg["n_ch"] * 2 * n_out)
            eng.dev_upload(d_in, piece)
            z.run_device(d_in, piece.shape[1] * B, d_out)
            eng.synchronize()
            got = eng.dev_download(d_out, cfg["n_ch"] * 2 * n_out).reshape(cfg["n_ch"], -1)
            eng.dev_free(d_in)
            eng.dev_free(d_out)
        else:
            got = z.run(piece)
        ctx.count("fmt ops", len(ops))
        ctx.count("fmt device calls" if device else "fmt host calls")
        want = sfm.channelize(epoch, fmt, cfg["h"], M, src[ck], inc[ck], shift[ck], P, m_range=(m0, m0 + n_out))
        for j, c in enumerate(ck):
            if not np.array_equal(got[c], want[j]):
                d = np.flatnonzero(got[c] != want[j])
                bad = ("call %d (%s form, %d outputs from output %d of the epoch): channel %d (source %d inc 0x%08x L %d) "
                       "differs in %d bytes, first at byte %d (outputs %s): got %s, model %s" % (
                           i, "device" if device else "host", n_out, m0, c, src[c], inc[c], shift[c], len(d), d[0],
                           np.unique(d // 2)[:12].tolist(), got[c][d[:8]].tolist(), want[j][d[:8]].tolist()))
                break
        if bad:
            break
    z.close()
    ctx.count("fmt cases")
    return bad


def fmt_case(rng, ctx, only=None):
    """only = "s8" / "s16": the case is drawn as ever and run if it is of that format (None otherwise, as if identical)."""
    cfg = draw_fmt(rng)
    if only is not None and cfg["fmt"] != only:
        return None
    bad = run_fmt(cfg, ctx)
    return None if bad is None else "format case: %s\n  %s" % (describe_fmt(cfg), bad)


def compute_units():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process: torch brings its own HIP
    runtime, which finds no device in a process where the engine's has opened it first."""
    import subprocess
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError("torch could not read the device's properties: " + r.stderr[-2000:])
    return int(r.stdout.split()[-1])


def fixed_scan_case(which, ctx, cus=None):
    """The two walker geometries no draw reaches cheaply.  "waves3": enough following tiles (3 per compute unit) for
    workgroups of three tiles and two waves per tile, at 256-byte engine blocks.  "window64": M = 64, K = 1024 - windows
    of 192 outputs - at 2048-byte engine blocks: 1024 = 5 x 192 + 64, a last window of 64 outputs."""
    rng = np.random.default_rng({"waves3": 31, "window64": 32}[which])
    if which == "waves3":
        n_ch = 3 * 8 * int(cus if cus else compute_units())
        M = 4
        check = sorted(rng.choice(n_ch, 24, replace=False).tolist())
        return run_scan(ctx, M, None, capi.channelizer_default_taps(M), 1, n_ch, 256, [3, 2], rng, check=check,
                        follow_p=1.1, what="fixed scan case waves3")
    h = rng.integers(-4000, 4001, 1024).astype(np.int16)
    check = sorted(rng.choice(40, 24, replace=False).tolist())
    return run_scan(ctx, 64, h, h, 2, 40, 2048, [1, 1], rng, check=check, what="fixed scan case window64")


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.default_rng(seed)
    from oracle import bindings
    ctx = Context(bindings.Oracle())
    mode, fmode, smode = os.environ.get("FUZZ_SCAN"), os.environ.get("FUZZ_FRAC"), os.environ.get("FUZZ_SURVEY")
    gmode = os.environ.get("FUZZ_GAIN") == "1"
    tmode = os.environ.get("FUZZ_FMT") == "1"
    kmode = os.environ.get("FUZZ_TRACK") == "1"

    def one():
        if gmode:                                          # (asked for: no draw decides it, the other kinds draw as ever)
            return False, gain_case(rng, ctx)
        if tmode:                                          # (asked for as well)
            return False, fmt_case(rng, ctx)
        if kmode:
            return False, track_case(rng, ctx)
        r = rng.random() if mode is None else 1.0
        scan = mode == "1" or (mode is None and r < 0.125)
        if scan:
            return scan, scan_case(rng, ctx)
        if smode == "1" or (smode is None and mode is None and r >= 0.9):
            return scan, survey_case(rng, ctx)
        frac = fmode == "1" or (fmode is None and r < 0.27)     # (FUZZ_SCAN=0 alone: plain cases only, as ever)
        return scan, (frac_case(rng, ctx) if frac else plain_case(rng, ctx))

    if os.environ.get("FUZZ_REPLAY"):
        rng.bit_generator.state = json.load(open(os.environ["FUZZ_REPLAY"]))
        _, bad = one()
        print("replayed case:", "identical to the model" if bad is None else "MISMATCH: " + bad)
        sys.exit(0 if bad is None else 1)
    t0, n_scan = time.time(), 0
    for case in range(cases):
        if case and case % 500 == 0:
            print("chan_fuzz: %d cases so far, %.0f s" % (case, time.time() - t0), flush=True)
        state0 = rng.bit_generator.state
        scan, bad = one()
        n_scan += scan
        if bad is not None:
            print("MISMATCH in case %d of seed %d: %s" % (case, seed, bad))
            path = os.environ.get("FUZZ_STATE", os.path.join("fuzz_out", "chan_fuzz_fail_state.json"))
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            json.dump(state0, open(path, "w"))
            print("generator state kept: FUZZ_REPLAY=%s python tools/chan_fuzz.py" % path)
            sys.exit(1)
    print("chan_fuzz: %d cases (%d of them scan cases%s) identical to the model in %.0f s (seed %d)"
          % (cases, n_scan, "".join(", %d %s" % (v, k) for k, v in ctx.stats.items()), time.time() - t0, seed))
    ctx.close()


if __name__ == "__main__":
    main()
