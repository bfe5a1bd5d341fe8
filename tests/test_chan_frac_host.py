"""CPU tier: the fractional-rate channelizer (include/iqdemod.h: "Fractional decimation") without a GPU - its numpy model
(tests/chan_frac_model.py) against the integer one and against a float64 ideal, the per-branch default prototype
(iqd_channelizer_default_taps_q), the mutation proof of the GPU test's inputs (tests/chan_frac_cases.py), and the
cross-compiled kernel's code object."""
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import chan_frac_cases as fc
from tests import chan_frac_model as fm
from tests import chan_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS_OUT = 256000.0


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


@pytest.mark.parametrize("M,K", [(2, 1), (3, 17), (8, 105), (5, 64), (10, 131), (64, 300)])
def test_den_1_is_the_integer_model(P, M, K):
    rng = np.random.default_rng(M * 100 + K)
    h = rng.integers(-8000, 8001, K).astype(np.int16)
    h[0] = 32639 if K < 64 else 8000
    for kind in ("random", "rails"):
        u = fc.stream(rng, 2 * M * 512, kind)
        for inc, L in ((0, 0), (1, 8), (2 ** 31, 3), (2 ** 31 - 1, 0), (2 ** 32 - 1, 8), (int(rng.integers(0, 2 ** 32)), 5)):
            want = cm.channel(u, h, M, inc, L, P)
            assert np.array_equal(fm.channel(u, h, M, 1, inc, L, P), want), (kind, inc, L)
            assert np.array_equal(fm.channel(u, h, M, 1, inc, L, P, m_range=(100, 300)), want[200:600])


def test_default_taps_q_with_den_1_are_the_integer_taps(capi):
    L = capi._lib()
    for M in range(2, 65):
        want = capi.channelizer_default_taps(M)
        for den in (0, 1):
            out = np.zeros(len(want) + 4, np.int16)
            assert L.iqd_channelizer_default_taps_q(M, den, out.ctypes.data, len(out)) == len(want)
            assert np.array_equal(out[:len(want)], want) and not out[len(want):].any(), (M, den)


def _admissible():
    return [(p, q) for q in (2, 4, 8) for p in range(2 * q, 64 * q + 1) if math.gcd(p, q) == 1]


def test_every_branch_of_every_default_prototype_has_unit_dc_gain(capi):
    ratios = _admissible()
    assert len(ratios) == 62 + 124 + 248 and set(fc.RATIOS) <= set(ratios)
    for p, q in ratios:
        h = capi.channelizer_default_taps(p, q).astype(np.int64)
        assert len(h) == 13 * p + 1 and -(-len(h) // q) <= 1024, (p, q)
        assert np.abs(h).max() <= 32639
        for r in range(q):
            assert int(h[r::q].sum()) == 32768, (p, q, r)
            assert 256 * int(np.abs(h[r::q]).sum()) <= 2 ** 31 - 256, (p, q, r)
        # the peak: 2 fc 32768 Q = 31744 Q / P, within the passband ripple (0.32 dB, 3.7 %), the 1.5 % by which the two
        # middle taps of an even-length prototype miss the sinc's top at P = 5, and the rounding
        assert abs(int(h.max()) - 31744 * q / p) <= 0.06 * 31744 * q / p + 2, (p, q, h.max())


def test_default_taps_q_refuses_inadmissible_ratios(capi):
    L = capi._lib()
    for p, q in ((75, 3), (75, 16), (6, 4), (12, 8), (3, 2), (15, 8), (129, 2), (513, 8), (1, 1), (65, 1), (0, 2)):
        assert L.iqd_channelizer_default_taps_q(p, q, None, 0) == -1, (p, q)
        with pytest.raises(capi.IqdError):
            capi.channelizer_default_taps(p, q) if q != 1 else capi.channelizer_default_taps(p)
    assert L.iqd_channelizer_default_taps_q(75, 8, None, 5) == -1          # a capacity without a buffer


@pytest.mark.parametrize("p,q", fc.RATIOS)
def test_default_prototype_meets_the_integer_prototypes_bounds(capi, p, q):
    """tests/test_chan_host.py's bounds on the quantised taps (ripple <= 0.5 dB over +-100 kHz, >= 50 dB down from
    156 kHz), measured at the prototype's own rate 256000 P.  Its DC gain is Q x 32768 (each branch's is 32768)."""
    h = capi.channelizer_default_taps(p, q).astype(np.int64)
    assert int(h.sum()) == 32768 * q
    assert np.abs(h - h[::-1]).max() <= 8          # symmetric up to each branch's rounding remainder
    w = np.fft.rfft(h.astype(np.float64), 1 << 18)
    f = np.fft.rfftfreq(1 << 18) * FS_OUT * p
    H = np.abs(w) / (32768.0 * q)
    pb, sb = H[f <= 100e3], H[f >= 156e3]
    ripple, stop = 20 * np.log10(pb.max() / pb.min()), -20 * np.log10(sb.max())
    print("P/Q = %d/%d: ripple %.3f dB, stopband %.1f dB" % (p, q, ripple, stop))
    assert ripple <= 0.5
    assert stop >= 50.0


def _tone(n, rate, f, amp=100.0):
    z = amp * np.exp(2j * np.pi * f * np.arange(n) / rate)
    u = np.empty(2 * n, np.uint8)
    u[0::2] = np.clip(np.rint(z.real) + 128, 0, 255)
    u[1::2] = np.clip(np.rint(z.imag) + 128, 0, 255)
    return u


def _ideal(u, h, p, q, inc, L):
    """float64: the mixed-down capture zero-stuffed to the rate 256000 P, filtered by h / 32768, every P-th sample from
    u = P - 1 on: y[m] = 2^L sum_k h[k Q + r] / 32768 v[n - k]."""
    x = (u[0::2].astype(np.float64) - 128) + 1j * (u[1::2].astype(np.float64) - 128)
    w = 2 * np.pi * np.int32(np.uint32(inc)).item() / 2.0 ** 32
    up = np.zeros(len(x) * q, complex)
    up[::q] = x * np.exp(-1j * w * np.arange(len(x)))
    return np.convolve(h.astype(np.float64) / 32768.0, up)[p - 1:len(up):p] * 2 ** L


@pytest.mark.parametrize("p,q,offset,delta,L", [
    (75, 8, 300e3, 12e3, 0), (75, 8, -640e3, -40e3, 2), (15, 2, 0.0, 25e3, 0), (45, 4, -1440e3, 10e3, 0),
    (25, 2, None, -10e3, 1), (5, 2, 100e3, 20e3, 0), (17, 8, -200e3, -70e3, 1),
])
def test_model_is_an_ideal_fractional_down_converter_within_one_lsb(capi, P, p, q, offset, delta, L):
    rate = FS_OUT * p / q
    h = capi.channelizer_default_taps(p, q)
    inc = 2 ** 31 - 1 if offset is None else capi.phase_inc(offset, rate)
    fc_hz = np.int32(np.uint32(inc)).item() / 2.0 ** 32 * rate
    n = 512 * p
    u = _tone(n, rate, fc_hz + delta, amp=100.0 / 2 ** L)
    y = fm.channel(u, h, p, q, inc, L, P).astype(np.int64) - 128
    yc = y[0::2] + 1j * y[1::2]
    ideal = _ideal(u, h, p, q, inc, L)
    assert len(yc) == 512 * q == len(ideal)
    settle = len(h) // p + 1
    err = np.abs(yc[settle:].real - ideal[settle:].real).max(), np.abs(yc[settle:].imag - ideal[settle:].imag).max()
    assert max(err) <= 1.0, err
    rot = np.angle(np.sum(yc[settle + 1:] * np.conj(yc[settle:-1])))
    assert abs(rot - 2 * np.pi * delta / FS_OUT) < 1e-2
    assert abs(np.abs(yc[settle:]).mean() - 100.0) < 3.5        # unity gain in the passband (0.32 dB ripple)


def test_out_of_band_tones_are_silence_and_empty_branches_are_0x80(capi, P):
    p, q = 75, 8
    rate = FS_OUT * p / q
    h = capi.channelizer_default_taps(p, q)
    inc = capi.phase_inc(200e3, rate)
    for delta in (160e3, 300e3):
        y = fm.channel(_tone(256 * p, rate, 200e3 + delta), h, p, q, inc, 0, P)
        assert (y[2 * 16:] == 128).all(), delta
    u = np.random.default_rng(3).integers(0, 256, 2 * 64 * 17, dtype=np.uint8)
    y = fm.channel(u, np.array([20000, -20000, 20000], np.int16), 17, 8, 12345, 4, P).reshape(-1, 2)
    r = (np.arange(len(y)) * 17 + 16) % 8
    assert (y[r >= 3] == 128).all() and (y[r < 3] != 128).any()


# the defects one case cannot see, and why
BLIND = {
    # one tap, h_0 = (h[0]): only the outputs of branch 0 are not 0x80, and there u mod Q = 0 (ceil = floor) and the only
    # tap delay is k = 0 on either grid
    "K1-5/2": {"n_ceil", "delay_q_grid"},
}


def test_every_gpu_input_sees_every_defect(capi, P):
    """The model with one defect switched on must differ from the spec on each case the GPU test runs (the unit-sized calls
    of its second pass are the call boundaries of call_restart), and every ratio of the list must see every defect."""
    seen = {}
    for c in fc.cases(capi):
        want = fm.channelize(c.wide, c.h, c.P, c.Q, c.src, c.inc, c.shift, P)
        assert (want == 0).any() and (want == 255).any(), c          # both byte rails
        blind = set()
        for mu in fm.MUTANTS:
            got = fm.channelize(c.wide, c.h, c.P, c.Q, c.src, c.inc, c.shift, P, mutant=mu, calls=c.calls)
            if np.array_equal(got, want):
                blind.add(mu)
            else:
                seen.setdefault((c.P, c.Q), set()).add(mu)
        assert blind == BLIND.get(c.name, set()), (c, blind)
    assert set(seen) == set(fc.RATIOS)
    for ratio, mus in seen.items():
        assert mus == set(fm.MUTANTS), (ratio, set(fm.MUTANTS) - mus)


def test_the_limit_cases_drive_both_rails_of_stage_a(capi):
    """sat16 is reached: with every branch's tap sum at the limit a full-scale stretch overflows int16 many times over."""
    for c in fc.cases(capi):
        if not c.name.startswith("limit"):
            continue
        for r, hr in enumerate(fm.branches(c.h, c.Q)):
            assert int(np.abs(hr).sum()) == fc.SUM_LIMIT, (c, r)
        x = c.wide[0].astype(np.int64)[0::2] - 128
        hr = fm.branches(c.h, c.Q)[0]
        A = np.convolve(hr, x)[len(hr):len(x)]
        a = (A + 128) >> 8
        assert a.min() < -32768 and a.max() > 32767


@pytest.fixture(scope="module")
def code_object():
    """iqd_chan.hip and iqd_chan_frac.hip cross-compiled for gfx950 (device only, the library's flags): {kernel: metadata}"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in ("iqd_chan", "iqd_chan_frac"):
            asm = os.path.join(tmp, name + ".s")
            cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
                   "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
                   os.path.join(csrc, name + ".hip")]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
            for blk in re.split(r"\n\s+- \.agpr_count:", open(asm).read())[1:]:
                kernel = re.search(r"\.name:\s+(\S+)", blk).group(1)
                meta[kernel] = {k: int(v) for k, v in re.findall(
                    r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", blk)}
    return meta


def test_code_object_has_no_private_segment_and_the_integer_kernels_keep_their_registers(code_object):
    frac = [k for k in code_object if "chz_frac_kernel" in k]
    assert len(frac) == 3 and len(code_object) == 8, sorted(code_object)      # Q = 2, 4, 8; the five of iqd_chan.hip
    for k, m in code_object.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
    for k in frac:
        assert code_object[k]["vgpr_count"] <= 128, (k, code_object[k])     # 512 threads keep their full occupancy
    integer = {k: m["vgpr_count"] for k, m in code_object.items() if "10chz_kernelILi" in k}
    assert integer == {"_ZN3iqd10chz_kernelILi8EEEvNS_9ChzLaunchE": 121, "_ZN3iqd10chz_kernelILi0EEEvNS_9ChzLaunchE": 60}, integer


def test_isa_lint_of_the_fractional_kernels():
    """(iqd_chan.hip itself: tests/test_chan_host.py and tests/test_chan_scan_host.py)"""
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_chan_frac.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 3 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
