"""CPU tier: the band spectrum (include/iqdemod.h: "Band spectrum") without a GPU - the mutation proof of the GPU test's
inputs (tests/spectrum_cases.py) on the numpy model (tests/spectrum_model.py), the library's host-only functions against
the formulas, the model against numpy's float64 FFT, and the cross-compiled kernels' code object."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import spectrum_cases as sc
from tests import spectrum_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# iqd_spectrum_full_scale of the default windows and their sums, as the specification's author computed them
P_FS = {64: 1032256, 128: 4129024, 256: 16516096, 512: 66048129, 1024: 264225025, 2048: 264192516}
W_SUM = {64: 524246, 1024: 8387986, 2048: 8387416}


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def models(P):
    """name -> (case, Model): every expected array is computed once"""
    return {c.name: (c, sm.Model(c.wide, c.fmt, c.N, c.F, c.w(P), P)) for c in sc.cases(P)}


def test_case_list_covers_what_the_kernel_can_get_wrong(models):
    cs = [c for c, _ in models.values()]
    assert {c.N for c in cs} >= {64, 128, 1024, 2048} and {c.F for c in cs} >= {1, 2, 3, 32}
    assert any(c.F > sc.CHUNK and c.F % sc.CHUNK for c in cs)          # more frames than a wave takes at once, and a rest
    assert {-(-(c.F % sc.CHUNK) // 16) for c in cs} >= {1, 2, 3, 4}     # every size of the last chunk, in 16-frame tiles
    assert {c.blocks for c in cs} >= {1, 2, 3} and {c.n_src for c in cs} == {1, 3} and {c.fmt for c in cs} == {"u8", "s8"}
    assert max(c.wide.nbytes for c in cs) == 2 * 1024 * 32              # the constant input; everything else <= 32 KiB
    assert sorted(c.wide.nbytes for c in cs)[-2] <= 32 * 1024


def blind(c, m, P):
    """the defects a case cannot see by construction"""
    out = {"hi_wrap"}                 # |v| <= 32639 holds for every window create accepts: hi never reaches 128 (below)
    w = c.w(P)
    if np.array_equal(w, w[::-1]):
        out.add("window_reversed")    # a symmetric window
    if c.n_src == 1:
        out.add("source_0")
    if c.blocks == 1:
        out.add("div_call")           # the call's frames are the block's
    p = sm.frame_power(*m.sums())
    if p.reshape(c.n_src, c.blocks, c.F, c.N).sum(axis=2).max() < 2 ** 32:
        out.add("sum_wrap")           # no block sum reaches 2^32
    if c.name == "N1024-quiet":       # x = 0: the power is 0 whatever the coefficients, the rounding and the blocks are
        out = set(sm.DEFECTS) - {"flip"}
    if c.name == "N1024-const-F32":   # a constant: one line at the centre, which a mirrored band and a phase turn keep
        out |= {"conjugate", "iq_swap"}
    if c.name == "N64-half-point":    # sum |x| = 32 on one rail: |A| <= 2^15 sqrt 2, a real input's symmetric band - only
        out |= {"conjugate", "iq_swap", "lo_unsigned"}    # stage a's rounding, the shift and the block structure show
    return out


def test_every_gpu_input_sees_every_defect(models, P):
    """The model with one defect switched on must change some expected entry of each case the GPU test runs, except where
    the case cannot see the defect by construction (blind() above).  a_round_low is a matter of chance outside the case
    planted for it: it shows only where a bin sum sits exactly on the half point, one value in 65536, so a case is held
    to neither answer there.  Every defect but hi_wrap is seen by some case."""
    seen = set()
    for c, m in models.values():
        want = m.power()
        assert want.shape == (c.n_src, c.blocks, c.N) and want.dtype == np.uint32
        unseen = {d for d in sm.DEFECTS if np.array_equal(m.power(d), want)}
        seen |= set(sm.DEFECTS) - unseen
        if c.name != "N64-half-point":
            unseen.discard("a_round_low")
            assert unseen == blind(c, m, P) - {"a_round_low"}, (c, unseen ^ blind(c, m, P))
        else:
            assert unseen == blind(c, m, P), (c, unseen ^ blind(c, m, P))
    assert seen == set(sm.DEFECTS) - {"hi_wrap"}


def test_hi_plane_stays_in_int8_at_the_window_limit_and_wraps_past_it(P):
    """hi_wrap cannot show inside the window's bounds: at |w| = 32639 the largest coefficient splits into hi = 127 (the
    model asserts it for every case).  Past the bound - a window create refuses - hi reaches 128 and the defect shows."""
    c, s = sm.coefficients(np.full(64, 32639), P, 64)
    assert max(np.abs(c).max(), np.abs(s).max()) == 32638 and ((c + 128) >> 8).max() == 127 and ((-s + 128) >> 8).max() == 127
    w = np.full(64, 32767)
    c, s = sm.coefficients(w, P, 64, bounds=False)
    assert ((c + 128) >> 8).max() == 128
    x = np.random.default_rng(5).integers(-128, 128, (1, 1, 64, 2))
    good = sm.bin_sums(c, s, x[..., 0], x[..., 1], bounds=False)
    bad = sm.bin_sums(c, s, x[..., 0], x[..., 1], "hi_wrap", bounds=False)
    assert not np.array_equal(good[0], bad[0])


def test_planted_cases_are_what_they_claim(models, P, capi):
    c, m = models["N64-half-point"]
    Ar, Ai = m.sums()
    assert Ar[0, 0, 32] == 2 ** 15 and Ar[0, 1, 32] == -2 ** 15 and Ai[0, :, 32].tolist() == [0, 0]
    assert m.power()[0, :, 32].tolist() == [1, 0] and m.power("a_trunc")[0, :, 32].tolist() == [0, 1]
    assert m.power("a_round_low")[0, :, 32].tolist() == [0, 1]
    c, m = models["N1024-const-F32"]
    want = m.power()
    assert want[0, 0, 512] == P_FS[1024] == capi.spectrum_full_scale(1024) and 32 * P_FS[1024] > 2 ** 32
    c, m = models["N1024-quiet"]
    assert not m.power().any() and m.power("flip").any()
    # the sign-matched rails reach the largest sums of the whole list, close to the bound 128 x 1.4143 x 2^23
    c, m = models["N1024-rails-8191-s8"]
    Ar, Ai = m.sums()
    assert Ar[0, 0, 700] == np.abs(Ar).max() > 0.85 * 128 * 1.4143 * 2 ** 23 and Ai[0, 1, 3] == np.abs(Ai).max() > 2 ** 30
    assert 256 * 1024 * 8191 <= 2 ** 31 - 256 < 256 * 1024 * 8192       # the rectangular window at the sum's limit
    c, m = models["N64-rails-32639"]
    Ar, Ai = m.sums()
    assert Ar[0, 0, 41] == np.abs(Ar).max() and Ai[0, 1, 9] == np.abs(Ai).max()
    c, _ = models["N64-F104-neg"]
    assert c.window.min() < 0 and not np.array_equal(c.window, c.window[::-1])


def test_default_window_and_full_scale_are_the_formulas(capi, P):
    for N in sm.N_SET:
        w, sh = sm.default_window(N, P)
        got = capi.spectrum_default_window(N)
        assert got.dtype == np.int16 and np.array_equal(got, w) and sh == (3 if N == 2048 else 2)
        assert np.array_equal(w, w[::-1]) and w.min() >= 0
        sm.check_window(w, N)
        if N in W_SUM:
            assert int(w.sum()) == W_SUM[N]
        assert capi.spectrum_full_scale(N) == sm.full_scale(w) == P_FS[N] == capi.spectrum_full_scale(N, w)
    # windows of the caller's, negative entries included; and full scale is bin N / 2 of the constant (255, 128)
    rng = np.random.default_rng(11)
    for N in (64, 256):
        w = rng.integers(-4000, 4001, N).astype(np.int16)
        assert capi.spectrum_full_scale(N, w) == sm.full_scale(w)
        const = np.tile(np.array([255, 128], np.uint8), N)[None]
        assert sm.spectrum(const, "u8", N, 1, w, P)[0, 0, N // 2] == sm.full_scale(w)
    assert np.allclose(capi.spectrum_dbfs([0, 1, P_FS[64], 10 * P_FS[64]], P_FS[64]),
                       [-10 * np.log10(P_FS[64])] * 2 + [0.0, 10.0])


def test_host_only_refusals(capi):
    L = capi._lib()
    out = np.zeros(4096, np.int16)
    p = C.c_uint32(7)
    for n in (0, 1, 32, 63, 65, 96, 192, 1000, 4096, 2 ** 31, 2 ** 32 - 64):
        assert L.iqd_spectrum_default_window(n, capi._np_ptr(out)) == -1, n
        assert L.iqd_spectrum_full_scale(None, n, C.byref(p)) == -1 and p.value == 7, n
        with pytest.raises(capi.IqdError):
            capi.spectrum_default_window(n)
        with pytest.raises(capi.IqdError):
            capi.spectrum_full_scale(n)
    assert not out.any()
    assert L.iqd_spectrum_default_window(64, None) == -1
    assert L.iqd_spectrum_full_scale(None, 64, None) == -1
    # a window outside its bounds: an entry past 32639 either way, the sum past (2^31 - 256) / 256
    w = np.zeros(64, np.int16)
    for bad in (32640, -32640, -32768):
        w[17] = bad
        with pytest.raises(capi.IqdError):
            capi.spectrum_full_scale(64, w)
    w[17] = -32639
    assert capi.spectrum_full_scale(64, w) == sm.full_scale(w)
    assert capi.spectrum_full_scale(1024, np.full(1024, 8191, np.int16)) == sm.full_scale(np.full(1024, 8191))
    for w in (np.full(1024, 8192, np.int16), np.full(1024, -8192, np.int16)):
        with pytest.raises(capi.IqdError):
            capi.spectrum_full_scale(1024, w)
    with pytest.raises(ValueError):
        capi.spectrum_full_scale(64, np.zeros(65, np.int16))


# model vs float64 FFT, measured on the committed cases: 0.43 dB above a mean power of 100 (the worst are the F = 1
# cases, where stage a's rounding of one frame's |a| = 10 by up to 0.5 is 0.42 dB by itself) and 0.050 dB above 10^4
FFT_TOL = {100: 2 * 0.43, 10 ** 4: 2 * 0.050}


def test_model_against_numpy_fft(models, P):
    """The model against numpy's float64 FFT of the same windowed frames, fftshifted and scaled by 32767 / 32768 / 65536:
    equal argmax on every tone, and dB agreement on the bins above a power floor.  Measured on these cases: at most
    0.43 dB above mean power 100 and 0.050 dB above 10^4; the bounds are twice that, as margin for other seeds (FFT_TOL).
    This checks the model against an independent FFT, never the device against itself."""
    worst = {f: 0.0 for f in FFT_TOL}
    for c, m in models.values():
        want = m.power().astype(np.float64)
        ref = sm.fft_power(c.wide, c.fmt, c.N, c.F, c.w(P))
        if c.tones:
            assert want[:, 0].argmax(axis=-1).tolist() == ref[:, 0].argmax(axis=-1).tolist() == c.tones
        for floor in FFT_TOL:
            sel = want > floor
            if sel.any():
                worst[floor] = max(worst[floor], np.abs(10 * np.log10(want[sel] / ref[sel])).max())
    print("model vs FFT, worst dB by floor:", worst)
    for floor, tol in FFT_TOL.items():
        assert 0 < worst[floor] <= tol, worst


@pytest.fixture(scope="module")
def code_object():
    """iqd_spectrum.hip cross-compiled for gfx950 (device only, the library's flags): {kernel: metadata}, the text"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "iqd_spectrum.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
               os.path.join(csrc, "iqd_spectrum.hip")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(asm).read()
        for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
            kernel = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[kernel] = {k: int(v) for k, v in re.findall(
                r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\d+)", blk)}
    return meta, text


def test_code_object(code_object):
    meta, text = code_object
    assert sorted(meta) == ["_ZN3iqd10spc_kernelILb0EEEvNS_9SpcLaunchE", "_ZN3iqd10spc_kernelILb1EEEvNS_9SpcLaunchE"]
    for k, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["group_segment_fixed_size"] == 0, (k, m)                    # no LDS
        assert m["vgpr_count"] == 152, (k, m)                                # 88 + 64 accumulators: 3 waves per SIMD
    # per kernel: the whole chunk of 4 frame tiles and the rests of 1 .. 4, four accumulators each
    assert text.count("v_mfma_i32_16x16x64_i8") == 2 * (4 + 4 + 3 + 2 + 1) * 4


def test_isa_lint_of_the_spectrum_kernels():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_spectrum.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 2 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
