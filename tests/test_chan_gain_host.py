"""CPU tier for gain-following wideband channels (include/iqdemod.h: iqd_channelizer_follow_gain): the dB step's identity
with the gain shift, the mantissa literals, the mutation proof of the GPU test's inputs (tests/chan_gain_cases.py) on the
numpy model (tests/chan_gain_model.py), and the cross-compiled walker's code object."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import chan_gain_cases as gc
from tests import chan_gain_model as gm
from tests import chan_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def cases(capi):
    got = gc.cases(capi)
    assert [c.name for c in got] == gc.case_names()
    return got


def test_gain_of_6_L_is_the_gain_shift_L(capi, P):
    rng = np.random.default_rng(11)
    for M in (2, 8):
        h = capi.channelizer_default_taps(M)
        wide = rng.integers(0, 256, 2 * 600 * M, dtype=np.uint8)
        wide[:8] = [0, 255, 255, 0, 0, 0, 255, 255]
        for L in range(9):
            inc = int(rng.integers(0, 2 ** 32))
            assert np.array_equal(gm.channel_db(wide, h, M, inc, 6 * L, P), cm.channel(wide, h, M, inc, L, P)), (M, L)
    # the arithmetic behind it, on every residue and both signs: floor(r / 4) + 2^(19-e) = floor((r + 2^(21-e)) / 4)
    r = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 100000), np.arange(-9, 10), [2 ** 31 - 1, -2 ** 31 + 1]]).astype(np.int64)
    for e in range(9):
        assert np.array_equal(((r * 4096 >> 14) + (1 << (19 - e))) >> (20 - e), (r + (1 << (21 - e))) >> (22 - e))


def test_mantissa_literals():
    want = [int(np.rint(4096 * 2 ** (j / 6))) for j in range(6)]
    assert list(gm.M_J) == want == [4096, 4598, 5161, 5793, 6502, 7298]
    hdr = open(os.path.join(ROOT, "include", "iqdemod.h")).read()
    assert [int(v) for v in re.findall(r"#define IQD_GAIN_M[0-5] (\d+)", hdr)] == want
    assert re.search(r"#define IQD_GAIN_FOLLOW_MAX (\d+)", hdr).group(1) == str(gm.G_MAX)
    assert all(m << 18 < 2 ** 31 for m in want)                        # the kernel's route: the high word of r (m_j 2^18)
    # a step of 1 in g is 20 log10(2) / 6 dB; the rounded mantissa keeps it within 0.001 dB
    for j in range(6):
        assert abs(20 * np.log10(want[j] / 4096) - j * 20 * np.log10(2) / 6) < 1e-3


# The defects a case cannot see, by construction.
AGC_ON = {"clamp46", "no_clamp",     # an AGC's gain starts at 24 and never exceeds MAX_ADJUSTIBLE_GAIN = 46
          "manual_ignored"}          # (the defect is about a disabled AGC)
AGC_OFF = {"late", "held", "early",  # the gain moves only between calls
           "m_trunc"}                # the manual gains the cases use, 0 5 6 24 47 48 60, have g mod 6 in {0, 5}, whose
#                                      mantissas 4096 and 7298 truncate to themselves
# t_trunc changes floor(r m / 2^14) by one for negative r, which reaches the byte only where t + 2^(19-e) lies just below a
# multiple of 2^(20-e): once in 2^(20-e) unsaturated negative samples, 2^13 at the highest gain an AGC reaches.  The cases
# with a handful of channels hold too few samples at high gain; K300's random full-scale input is saturated there.
BLIND = {
    "M8-1ch-harris": AGC_ON | {"t_trunc", "ch0_gain",   # one channel
                               "sat127"},               # the weak carrier alone: no output reaches -128
    "M8-7ch-lowpass": AGC_ON | {"t_trunc"},
    "M2-9ch-harris": AGC_ON | {"t_trunc"},
    "M7-65ch-harris": AGC_ON,
    "M8-7ch-off": AGC_OFF,
    "K300-9ch-off": AGC_OFF | {"t_trunc"},
    "M8-2win-harris": AGC_ON,
}


def test_every_gpu_input_sees_every_defect(P, cases):
    from oracle.bindings import Oracle
    o = Oracle()
    seen_anywhere = set()
    for case in cases:
        fol = [int(c) for c in np.nonzero(case.follow)[0]]
        rots = {c: gm.rotated(case.wide[int(case.src[c])], case.h, case.M, int(case.inc[c]), P) for c in fol}
        truth = {c: gc.run_model(gm, o, case, P, c, rot=rots[c]) for c in fol}
        g0 = truth[fol[0]][4]                      # "channel 0": the first following channel
        seen = set()
        for d in gm.DEFECTS:
            for c in fol:
                w = gc.run_model(gm, o, case, P, c, defect=d, gains0=g0, rot=rots[c])
                if any(not np.array_equal(np.concatenate(a), np.concatenate(b)) for a, b in zip(w, truth[c])):
                    seen.add(d)
                    break
        assert set(gm.DEFECTS) - seen == BLIND[case.name], (case.name, (set(gm.DEFECTS) - seen) ^ BLIND[case.name])
        seen_anywhere |= seen
    assert seen_anywhere == set(gm.DEFECTS)


def test_the_cases_reach_what_they_are_for(capi, P, cases):
    from oracle.bindings import Oracle
    o = Oracle()
    by = {c.name: c for c in cases}
    assert {c.M for c in cases} >= {2, 7, 8} and {int(c.follow.sum()) for c in cases} >= {1, 7, 9, 65}
    assert {c.bb for c in cases} >= {256, 1024} and {c.agc for c in cases} == {None, 0, 1}
    assert (len(by["K300-9ch-off"].h) + 31) // 32 > 8                  # more K-chunks than stay in registers
    c = by["M2-9ch-harris"]
    assert c.n_src == 3 and 1 not in set(c.src[c.follow].tolist()) and 1 in set(c.src.tolist())   # a source with fixed channels only
    assert sum(1 for c in cases if not c.follow.all()) >= 4            # fixed channels beside following ones
    for c in cases:
        assert c.calls[-1] < c.bb and c.calls[-1] % 64 == 0 and all(n % c.bb == 0 for n in c.calls[:-1]), c.name
        assert c.wide.shape == (c.n_src, sum(c.calls) * c.M)
    c = by["M8-2win-harris"]                                           # a block of more outputs than one window holds
    assert c.bb // 2 > capi.channelizer_window_outputs(c.M, len(c.h)) and c.bb // 2 % capi.channelizer_window_outputs(c.M, len(c.h))
    assert {g for k in by["M8-7ch-off"].manual.values() for g in k.values()} == set(gc.MANUAL) == {0, 5, 6, 24, 47, 48, 60}
    assert by["K300-9ch-off"].wide.min() == 0 and by["K300-9ch-off"].wide.max() == 255
    # the loops settle where the CPU run of the issue put them: the weak carrier near 26 dB, the medium one at 14, the
    # strong one pinned at 0; a free frequency runs to the rail region; the gain moves over several blocks on the way
    c = by["M7-65ch-harris"]
    fol = [int(x) for x in np.nonzero(c.follow)[0]]
    ends = set()
    for ch in fol[:12]:
        g = np.concatenate(gc.run_model(gm, o, c, P, ch)[4])
        ends.add(int(g[-1]))
        assert len(set(g[:12].tolist())) >= 2, ch
    assert 0 in ends and 14 in ends and ends & {25, 26, 27} and max(ends) >= 38, ends
    rows = np.concatenate(gc.run_model(gm, o, by["K300-9ch-off"], P, int(np.nonzero(by["K300-9ch-off"].follow)[0][3]))[0])
    assert rows.min() == 0 and rows.max() == 255                        # the output's rails at high gain


@pytest.fixture(scope="module")
def code_object():
    """iqd_chan_gain.hip cross-compiled for gfx950 (device only, the library's flags): {kernel: metadata}"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "iqd_chan_gain.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
               os.path.join(csrc, "iqd_chan_gain.hip")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        for blk in re.split(r"\n\s+- \.agpr_count:", open(asm).read())[1:]:
            kernel = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[kernel] = {k: int(v) for k, v in re.findall(
                r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", blk)}
    return meta


def test_code_object_of_the_gain_walker(code_object):
    assert sorted(code_object) == ["_ZN3iqd15chz_gain_kernelILi0EEEvNS_9ChzLaunchENS_13ChzGainLaunchE",
                                   "_ZN3iqd15chz_gain_kernelILi8EEEvNS_9ChzLaunchENS_13ChzGainLaunchE"]
    for k, m in code_object.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["vgpr_count"] <= 256, (k, m)                             # 512 threads per workgroup
    got = {re.search(r"ILi(\d)E", k).group(1): code_object[k]["vgpr_count"] for k in code_object}
    assert got == {"8": 145, "0": 80}, got


def test_isa_lint_of_the_gain_walker():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_chan_gain.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 2 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
