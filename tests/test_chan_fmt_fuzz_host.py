"""CPU tier: the fixed slice of tools/chan_fuzz.py's format cases (signed captures; SLICES["fmt"], run on the GPU by
tests/test_gpu_chan_fmt_fuzz.py) is worth running - its checked channels expose every defect of tests/chan_fmt_model.py, it
reaches the edges of chz_fmt_kernel and of the host code around it, and the model it is compared with gives the U8 model's
bytes for the same signal at the drawn M, K and increments.

N = 36 cases of seed 9106 (22 S8, 14 S16): case 29 is the last that is the first to reach something of REQUIRED below (S16
at M = 2), and every defect has been exposed twice by case 17; the six cases after 29 are the margin.  The case that first
exposes each defect, S8 / S16 ("-": not that format's):
    lo_signed - / 4      no_g - / 0        g_sign - / 0      big_endian - / 0     round_m1 2 / 0     trunc 1 / 0
    wrap32 - / 14        s8_flip 1 / -     hist_lo0 - / 0    hist_short 2 / 0     iq_swap 1 / 0
(wrap32 needs a case on the taps' limit, lo_signed an input whose low byte is not 256 x an 8-bit value's.)"""
import glob
import os
import re
import sys

import numpy as np
import pytest

from tests import chan_fmt_model as fm
from tests import chan_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N = 36
LAST_FIRST = 29            # the last case that is the first to reach something of REQUIRED or to expose a defect
# what the slice runs, per format: tests/test_gpu_chan_fmt_fuzz.py asserts at least these of the GPU run's counters
COUNTS = {"s8": {"fmt cases": 22, "fmt device calls": 50, "fmt host calls": 35, "fmt ops": 35},
          "s16": {"fmt cases": 14, "fmt device calls": 30, "fmt host calls": 35, "fmt ops": 27}}


@pytest.fixture(scope="module")
def chan_fuzz():
    import chan_fuzz as cf
    return cf


@pytest.fixture(scope="module")
def P(chan_fuzz):
    return chan_fuzz.ctx_phasor()


@pytest.fixture(scope="module")
def drawn(chan_fuzz):
    seed, n = chan_fuzz.SLICES["fmt"]
    assert (seed, n) == (9106, N)
    rng = np.random.default_rng(seed)
    return [chan_fuzz.draw_fmt(rng) for _ in range(n)]


def steps(chan_fuzz, cfg):
    """walk(cfg) with the samples per call of the epoch so far (chan_fmt_model's calls=) added to each step"""
    sizes = []
    for i, device, ops, epoch, m0, n_out, src, inc, shift in chan_fuzz.walk(cfg):
        if any(op[0] == "reset" for op in ops):
            sizes = []
        sizes = sizes + [n_out * cfg["M"]]
        assert sum(sizes) == epoch.shape[1] // 2 and m0 * cfg["M"] == sum(sizes[:-1])
        yield i, device, ops, epoch, m0, n_out, src, inc, shift, sizes


def test_every_defect_is_exposed_by_a_checked_channel(chan_fuzz, P, drawn, capsys):
    exposed = {"s8": {}, "s16": {}}                             # defect -> the cases that expose it (the first two)
    for case, cfg in enumerate(drawn):
        fmt, ck = cfg["fmt"], cfg["check"]
        todo = {d for d in fm.DEFECTS if fm.applies(d, fmt) and len(exposed[fmt].get(d, [])) < 2}
        for _, _, _, epoch, m0, n_out, src, inc, shift, sizes in steps(chan_fuzz, cfg):
            if not todo:
                break
            args = (epoch, fmt, cfg["h"], cfg["M"], src[ck], inc[ck], shift[ck], P)
            want = fm.channelize(*args, m_range=(m0, m0 + n_out))
            assert want.shape == (len(ck), 2 * n_out)
            for d in sorted(todo):
                if not np.array_equal(want, fm.channelize(*args, defect=d, calls=sizes, m_range=(m0, m0 + n_out))):
                    exposed[fmt].setdefault(d, []).append(case)
                    todo.discard(d)
    with capsys.disabled():
        for fmt in exposed:
            print("\nformat slice, %s: defect -> the first two cases that expose it: %r" % (fmt, exposed[fmt]))
    for fmt in ("s8", "s16"):
        want = {d for d in fm.DEFECTS if fm.applies(d, fmt)}
        assert set(exposed[fmt]) == want, (fmt, want - set(exposed[fmt]))
        assert all(len(v) == 2 for v in exposed[fmt].values()), (fmt, exposed[fmt])     # the margin: never one case alone
    assert max(v[0] for e in exposed.values() for v in e.values()) <= LAST_FIRST


def nq_reg():
    """CHZ_NQ_REG, read from the kernels' headers"""
    for path in sorted(glob.glob(os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_chan*.h"))):
        m = re.search(r"\bCHZ_NQ_REG\s*=\s*(\d+)\s*;", open(path).read())
        if m:
            return int(m.group(1))
    raise AssertionError("CHZ_NQ_REG not found")


def features(chan_fuzz, cfg, reg, P):
    """(what of the list below this case reaches, its counters as run_fmt counts them)"""
    f, M, K = cfg["fmt"], cfg["M"], cfg["K"]
    kp = (K + 31) // 32 * 32
    hsum = int(np.abs(cfg["h"].astype(np.int64)).sum())
    assert cfg["wide"].dtype == fm.DTYPE[f] and cfg["wide"].shape == (cfg["n_src"], sum(c["units"] for c in cfg["calls"]) * 64 * M)
    assert cfg["window"] == chan_fuzz.capi.channelizer_window_outputs(M, K, f) >= 64
    assert 2 <= M <= 64 and 1 <= K <= 1024 and 1 <= len(cfg["calls"]) <= 8 and 256 * hsum <= 2 ** 31 - 256
    checked = set(cfg["check"].tolist())
    assert {0, cfg["n_ch"] - 1} <= checked
    got = {f, "M=%d" % M, f + (" nq <= CHZ_NQ_REG" if kp // 32 <= reg else " nq > CHZ_NQ_REG")}
    got |= {f + " input " + k.split()[0] for k in cfg["kinds"]}
    got |= {f + " K <= 32"} if K <= 32 else {f + " K = 1023 or 1024"} if K >= 1023 else set()
    got |= {f + " M=%d" % M} if M in (2, 64) else set()
    got |= {f + " taps at the bound"} if 256 * hsum == 2 ** 31 - 256 and not cfg["limit"] else set()
    got |= {f + " limit"} if cfg["limit"] else set()
    got |= {f + " planted"} if cfg["planted"] else set()
    counts = dict.fromkeys(COUNTS[f], 0)
    counts["fmt cases"] = 1
    with_channel, before = set(cfg["src"].tolist()), cfg["inc"]
    for i, device, ops, epoch, m0, n_out, src, inc, shift, sizes in steps(chan_fuzz, cfg):
        counts["fmt ops"] += len(ops)
        counts["fmt device calls" if device else "fmt host calls"] += 1
        if n_out > cfg["window"]:
            got.add(f + " a call of several windows")
            if n_out % cfg["window"] == 32:
                got.add(f + " a last window of 32 outputs")
        if n_out == 32 and m0 > 0:                               # (m0 > 0: the history holds an earlier call's bytes)
            got.add(f + " a 32-output call after a call")
        if m0 > 0 and n_out * M < kp:                            # the history kernel keeps some of the history's own bytes
            got.add(f + " a call shorter than the history")
        for op in ops:
            got.add(f + " " + op[0])
            if op[0] == "move" and op[2] not in with_channel and op[1] in checked:
                got.add(f + " a source gets its first channel by a move")
            past = sorted(set(range(max(8, op[1]), op[1] + len(op[2]))) & checked) if op[0] == "retune" else []
            if past:                                             # (channels >= 8: not in tile 0 whatever the grouping)
                got.add(f + " a retune past the first tile")
                args = (epoch, f, cfg["h"], M, src[past], inc[past], shift[past], P)
                if f == "s16" and not np.array_equal(fm.channelize(*args, m_range=(m0, m0 + n_out)),
                                                     fm.channelize(*args, m_range=(m0, m0 + n_out), stale_g=before[past])):
                    got.add(f + " a retune past the first tile that shows if its coefficient sums stay the old ones")
        with_channel |= set(src.tolist())
        before = inc
    return got, counts


REQUIRED = (["M=2", "M=64", "s16 a retune past the first tile", "s16 M=2", "s16 M=64",
             "s16 a retune past the first tile that shows if its coefficient sums stay the old ones"] +
            [f + what for f in ("s8", "s16") for what in (
                "", " nq <= CHZ_NQ_REG", " nq > CHZ_NQ_REG", " K <= 32", " K = 1023 or 1024", " a call of several windows",
                " a last window of 32 outputs", " a 32-output call after a call", " a call shorter than the history",
                " retune", " move", " reset", " form", " a source gets its first channel by a move", " taps at the bound",
                " limit", " planted", " input full", " input small", " input rails", " input constant", " input carriers")])


def test_the_slice_reaches_the_edges(chan_fuzz, P, drawn, capsys):
    reg = nq_reg()
    first, counts = {}, {f: dict.fromkeys(COUNTS[f], 0) for f in COUNTS}
    for case, cfg in enumerate(drawn):
        got, n = features(chan_fuzz, cfg, reg, P)
        for k in got:
            first.setdefault(k, case)
        for k, v in n.items():
            counts[cfg["fmt"]][k] += v
    missing = [k for k in REQUIRED if k not in first]
    with capsys.disabled():
        print("\nformat slice: %d edges reached, the last of them first by case %d of %d; %r" % (
            len(REQUIRED) - len(missing), max(first[k] for k in REQUIRED if k in first), N, counts))
    assert not missing, missing
    late = {k: first[k] for k in REQUIRED if first[k] > LAST_FIRST}
    assert not late, late                                        # the cases after LAST_FIRST are the margin
    assert counts == COUNTS, counts
    # the limit cases reach sat16 at both ends on their first channel's source (the input is matched to its increment)
    for f in ("s8", "s16"):
        cfg = next(c for c in drawn if c["limit"] and c["fmt"] == f)
        a = fm.channelize(cfg["wide"], f, cfg["h"], cfg["M"], cfg["src"][:1], cfg["inc"][:1], cfg["shift"][:1], P, stage_a=True)[0]
        assert {a.real.max(), a.imag.max()} == {32767} and {a.real.min(), a.imag.min()} == {-32768}, f


def test_the_format_is_neutral_for_equivalent_signals(chan_fuzz, P):
    """S16 of 256 (u8 - 128) and S8 of u8 ^ 0x80 give chan_model's bytes for u8, at the drawn M, K and increments: the
    first ten cases of the slice's seed (the slice and the cases after it) with a carrier source that has channels, up to
    three of its channels, its first 128 outputs"""
    done = 0
    rng = np.random.default_rng(chan_fuzz.SLICES["fmt"][0])
    for cfg in (chan_fuzz.draw_fmt(rng) for _ in range(3 * N)):
        on = [(s, np.flatnonzero(cfg["src"] == s)[:3]) for s in sorted(cfg["u8"]) if (cfg["src"] == s).any()]
        if not on or done == 10:
            continue
        s, chs = on[0]
        M = cfg["M"]
        u8 = cfg["u8"][s][:2 * M * min(128, len(cfg["u8"][s]) // (2 * M))]
        want = np.stack([cm.channel(u8, cfg["h"], M, int(cfg["inc"][c]), int(cfg["shift"][c]), P) for c in chs])
        for fmt in ("s8", "s16"):
            got = fm.channelize(fm.from_u8(u8, fmt)[None], fmt, cfg["h"], M, [0] * len(chs), cfg["inc"][chs], cfg["shift"][chs], P)
            assert np.array_equal(got, want), (fmt, M, cfg["K"], chs)
        done += 1
    assert done == 10
