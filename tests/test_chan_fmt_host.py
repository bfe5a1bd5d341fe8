"""CPU tier: the channelizer on signed captures (include/iqdemod.h: "Signed captures") without a GPU - the mutation proof of
the GPU test's inputs (tests/chan_fmt_cases.py) on the numpy model (tests/chan_fmt_model.py), the model against the U8
model (tests/chan_model.py), the window formula at every M, and the cross-compiled kernels' code object."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import chan_fmt_cases as fc
from tests import chan_fmt_model as fm
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
    got = fc.cases(capi)
    assert [c.name for c in got] == fc.case_names()
    return got


def blind(c):
    """the defects a case cannot see by construction"""
    out = {d for d in fm.DEFECTS if not fm.applies(d, c.fmt)}          # the other format's
    if c.kind in ("small", "tiny"):
        out.add("wrap32")                          # small input or small taps: |A| < 2^31
    if len(c.h) == 1 or all(int(d) == 0 for d in c.inc):
        out.add("g_sign")                          # gi = 0 on every tap (tap 0 alone, or increment 0): sum gi = 0
    if len(c.h) == 1:
        out |= {"hist_lo0", "hist_short"}          # one tap: no history is read
    if c.kind == "limit":
        # the input sits on the rails and is matched to the taps: outside the few outputs where a segment's sums pass
        # through zero every |a| is far beyond what the output byte holds, so one unit of a, 128 per history sample or
        # half the taps' reach do not show
        out |= {"round_m1", "trunc", "hist_lo0", "hist_short"}
    return out


def test_every_gpu_input_sees_every_defect(P, cases):
    seen = {"s8": set(), "s16": set()}
    for c in cases:
        assert c.wide.dtype == fm.DTYPE[c.fmt] and c.wide.shape[0] == c.n_src
        assert sum(c.calls) == c.wide.shape[1] // 2 and all(n % (32 * c.M) == 0 for n in c.calls)
        kp = (len(c.h) + 31) // 32 * 32
        assert c.calls.count(32 * c.M) >= -(-kp // (32 * c.M)) + 2     # the chain of shortest calls
        want = fm.channelize(c.wide, c.fmt, c.h, c.M, c.src, c.inc, c.shift, P, calls=c.calls)
        assert np.array_equal(want, fm.channelize(c.wide, c.fmt, c.h, c.M, c.src, c.inc, c.shift, P)), c.name
        unseen = set(blind(c))
        for d in fm.DEFECTS:
            if not fm.applies(d, c.fmt):
                continue
            if np.array_equal(want, fm.channelize(c.wide, c.fmt, c.h, c.M, c.src, c.inc, c.shift, P, defect=d, calls=c.calls)):
                unseen.add(d)
            else:
                seen[c.fmt].add(d)
                assert d not in blind(c), (c.name, d)
        assert unseen == blind(c), (c.name, unseen ^ blind(c))
    assert seen["s16"] == {d for d in fm.DEFECTS if fm.applies(d, "s16")}
    assert seen["s8"] == {d for d in fm.DEFECTS if fm.applies(d, "s8")}


def test_the_cases_reach_what_they_are_for(capi, P, cases):
    by = {c.name: c for c in cases}
    assert {c.M for c in cases} >= {2, 7, 8, 64} and {len(c.src) for c in cases} >= {1, 7, 9, 65}
    c = by["M2-9ch-s16"]
    assert c.n_src == 3 and 1 not in set(c.src.tolist())               # a source without channels
    assert (len(by["K300-s16"].h) + 31) // 32 > 8                      # more K-chunks than stay in registers
    for c in cases:
        assert {0, 8} <= set(c.shift.tolist()) or len(c.src) < 3, c.name
        t = fc.window_outputs(c.M, len(c.h), c.fmt)
        n_out = c.wide.shape[1] // 2 // c.M
        assert n_out <= 4500
        if c.taps is None:                                             # whole windows and a 32-output tail
            assert n_out % t == 32 and n_out > t, c.name
    assert set(fc.EDGE_INCS) <= set(by["M8-65ch-s16"].inc.tolist())
    # small input: its 8-bit truncation (the high byte) is silence but for the planted samples
    w = by["M8-65ch-s16"].wide
    assert (np.abs(w.astype(np.int64)) <= 100).mean() > 0.999
    # the limit case: taps exactly at the limit; Lo leaves int32; sat16 at both ends on both rails
    c = by["limit-s16"]
    assert 256 * int(np.abs(c.h.astype(np.int64)).sum()) == 2 ** 31 - 256
    a = fm.channelize(c.wide, c.fmt, c.h, c.M, c.src, c.inc, c.shift, P, stage_a=True)
    for ch in range(len(c.src)):
        assert a[ch].real.max() == 32767 and a[ch].real.min() == -32768, ch
        assert a[ch].imag.max() == 32767 and a[ch].imag.min() == -32768, ch
    worst = 0
    for ch in range(1, 5):                                             # the diagonals
        gr, gi = cm.channel_taps(c.h, int(c.inc[ch]), P)
        u = c.wide[ch].astype(np.int64) & 0xff                         # the low bytes
        lo_r, lo_i = u[0::2] - 128, u[1::2] - 128
        n = np.arange(c.wide.shape[1] // 2 // c.M) * c.M + c.M - 1
        K = len(gr)
        Xr = np.lib.stride_tricks.sliding_window_view(np.concatenate([np.full(K - 1, -128), lo_r]), K)[n][:, ::-1]
        Xi = np.lib.stride_tricks.sliding_window_view(np.concatenate([np.full(K - 1, -128), lo_i]), K)[n][:, ::-1]
        Lo_r = Xr @ gr - Xi @ gi + 128 * (gr.sum() - gi.sum())
        Lo_i = Xi @ gr + Xr @ gi + 128 * (gr.sum() + gi.sum())
        worst = max(worst, int(np.abs(Lo_r).max()), int(np.abs(Lo_i).max()))
    assert worst > 1.39 * 2 ** 31, worst / 2 ** 31


def test_the_nested_shifts_are_the_spec():
    """the kernel's a = (H + ((Lo + 2^15) >> 8)) >> 8 is (256 H + Lo + 2^15) >> 16, and its value enters chz_epilogue as a
    high plane with a zero low one: (256 v + 128) >> 8 = v"""
    rng = np.random.default_rng(3)
    H = np.concatenate([rng.integers(-2 ** 31, 2 ** 31, 100000), [-2 ** 31, 2 ** 31 - 1, 0, -1]]).astype(np.int64)
    Lo = np.concatenate([rng.integers(-3 * 2 ** 30, 3 * 2 ** 30, 100000), [3 * 2 ** 30, -3 * 2 ** 30, -1, 0]]).astype(np.int64)
    v = (H + ((Lo + 2 ** 15) >> 8)) >> 8
    assert np.array_equal(v, (256 * H + Lo + 2 ** 15) >> 16)
    assert np.array_equal((256 * v + 128) >> 8, v)


@pytest.mark.parametrize("M", [2, 7, 8, 64])
def test_model_of_the_same_signal_is_the_u8_model(capi, P, M):
    """S16 of 256 (u8 - 128) and S8 of u8 ^ 0x80 give chan_model's bytes for u8"""
    rng = np.random.default_rng(M)
    h = capi.channelizer_default_taps(M)
    u8 = rng.integers(0, 256, (2, 2 * 96 * M), dtype=np.uint8)
    u8[0, :4] = [0, 255, 255, 0]
    src, inc, shift = fc.channel_set(rng, 6, [0, 1])
    want = cm.channelize(u8, h, M, src, inc, shift, P)
    for fmt in ("s8", "s16"):
        got = fm.channelize(fm.from_u8(u8, fmt), fmt, h, M, src, inc, shift, P)
        assert np.array_equal(got, want), fmt


def test_default_taps_keep_dc_unity(capi, P):
    """full-scale DC in, 127 out at L = 0 (and the negative rail: -128), on both formats"""
    for M in (2, 8, 64):
        h = capi.channelizer_default_taps(M)
        for fmt in ("s8", "s16"):
            info = np.iinfo(fm.DTYPE[fmt])
            w = np.zeros((1, 2 * 64 * M), fm.DTYPE[fmt])
            w[0, 0::2], w[0, 1::2] = info.max, info.min
            out = fm.channelize(w, fmt, h, M, [0], [0], [0], P)[0]
            assert out[-2] == 127 + 128 and out[-1] == 0, (M, fmt, out[-2:])


def test_window_formula_fits_lds_at_every_decimation(capi):
    """iqd_channelizer_window_outputs against the documented formula, and the window it gives against the LDS budget: both
    planes of an S16 window count"""
    for M in range(2, 65):
        for K in (1, len(capi.channelizer_default_taps(M)), 1024):
            kp = (K + 31) // 32 * 32
            for fmt, planes in (("u8", 1), ("s8", 1), ("s16", 2)):
                t = capi.channelizer_window_outputs(M, K, fmt)
                assert t == fc.window_outputs(M, K, "s8" if fmt == "u8" else fmt), (M, K, fmt)
                assert t % 64 == 0 and 64 <= t <= 1024, (M, K, fmt, t)
                assert 2 * planes * (t * M + kp) <= 32768, (M, K, fmt, t)
    assert capi.channelizer_window_outputs(64, 13 * 64 + 1, "s16") >= 32
    assert capi.channelizer_window_outputs(1, 1, "u8") == 0 and capi.channelizer_window_outputs(8, 1025, "s16") == 0


def test_config_keeps_its_layout(capi):
    import ctypes as C
    cfg = capi.ChannelizerConfig
    assert C.sizeof(cfg) == 40 and cfg.sample_format.offset == 28 and cfg.reserved.offset == 32 and cfg.reserved.size == 8
    assert cfg.decimation_den.offset == 24 and cfg.taps.offset == 16


@pytest.fixture(scope="module")
def code_object():
    """iqd_chan_fmt.hip cross-compiled for gfx950 (device only, the library's flags): {kernel: metadata}"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "iqd_chan_fmt.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
               os.path.join(csrc, "iqd_chan_fmt.hip")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        for blk in re.split(r"\n\s+- \.agpr_count:", open(asm).read())[1:]:
            kernel = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[kernel] = {k: int(v) for k, v in re.findall(
                r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", blk)}
    return meta


def test_code_object_has_no_private_segment_and_keeps_full_occupancy(code_object):
    fmt = [k for k in code_object if "chz_fmt_kernel" in k]
    assert len(fmt) == 4 and len(code_object) == 4, sorted(code_object)   # (planes 1, 2) x (registers, L2); the history kernel is iqd_chan.hip's
    for k, m in code_object.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["vgpr_count"] <= 128, (k, m)                             # 512 threads per workgroup
    got = {re.search(r"ILi(\d)ELi(\d)E", k).groups(): code_object[k]["vgpr_count"] for k in fmt}
    assert got == {("1", "8"): 121, ("1", "0"): 60, ("2", "8"): 121, ("2", "0"): 65}, got


def test_isa_lint_of_the_format_kernels():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_chan_fmt.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 4 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
