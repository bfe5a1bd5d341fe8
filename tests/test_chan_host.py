"""CPU tier: the wideband channelizer's host-only pieces (include/iqdemod.h: iqd_channelizer_phasor_table,
iqd_channelizer_default_taps), its integer spec (tests/chan_model.py) against a float64 ideal down-converter, and the
ISA lint of its kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import chan_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS_OUT = 256000.0


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


def test_phasor_table_is_the_formula(capi):
    P = capi.channelizer_phasor_table()
    assert P.shape == (4096, 2) and P.dtype == np.int16
    assert np.array_equal(P, cm.phasor_formula())


@pytest.mark.parametrize("M", [2, 4, 8, 10, 16, 64])
def test_default_taps_meet_their_spec(capi, M):
    h = capi.channelizer_default_taps(M).astype(np.int64)
    K = len(h)
    assert K % 2 == 1 and K <= 1024 and abs(K - (13 * M + 1)) <= M
    assert np.array_equal(h, h[::-1])
    assert np.abs(h).max() <= 32639 and 256 * np.abs(h).sum() <= 2 ** 31 - 256
    assert abs(int(h.sum()) - 32768) <= K // 2
    w = np.fft.rfft(h.astype(np.float64), 1 << 18)
    f = np.fft.rfftfreq(1 << 18) * FS_OUT * M
    H = np.abs(w) / 32768.0
    pb, sb = H[f <= 100e3], H[f >= 156e3]
    assert 20 * np.log10(pb.max() / pb.min()) <= 0.5
    assert -20 * np.log10(sb.max()) >= 50.0


def test_default_taps_refuse_bad_decimation(capi):
    L = capi._lib()
    for M in (0, 1, 65):
        assert L.iqd_channelizer_default_taps(M, None, 0) == -1


def _tone(n, rate, f, amp=100.0):
    t = np.arange(n)
    z = amp * np.exp(2j * np.pi * f * t / rate)
    u = np.empty(2 * n, np.uint8)
    u[0::2] = np.clip(np.rint(z.real) + 128, 0, 255)
    u[1::2] = np.clip(np.rint(z.imag) + 128, 0, 255)
    return u


def _ideal(u, h, M, inc, L):
    """float64 down-converter: y[m] = 2^L sum_k h[k] / 32768 x[n-k] e^{-j w (n-k)}, n = m M + M - 1."""
    x = (u[0::2].astype(np.float64) - 128) + 1j * (u[1::2].astype(np.float64) - 128)
    w = 2 * np.pi * np.int32(np.uint32(inc)).item() / 2.0 ** 32
    v = x * np.exp(-1j * w * np.arange(len(x)))
    y = np.convolve(h.astype(np.float64) / 32768.0, v)[M - 1:len(x):M]
    return y * 2 ** L


@pytest.mark.parametrize("M,offset,delta,L", [
    (8, 300e3, 12e3, 0), (8, -640e3, -40e3, 2), (4, 0.0, 25e3, 0), (10, 0.0, -70e3, 1),
    (8, -1024e3, 10e3, 0),               # -Fs/2 exactly (d = 2^31)
    (8, None, -10e3, 0),                 # just below +Fs/2 (d = 2^31 - 1)
])
def test_model_is_an_ideal_down_converter_within_one_lsb(capi, M, offset, delta, L):
    rate = FS_OUT * M
    P = capi.channelizer_phasor_table()
    h = capi.channelizer_default_taps(M)
    inc = 2 ** 31 - 1 if offset is None else capi.phase_inc(offset, rate)
    fc = np.int32(np.uint32(inc)).item() / 2.0 ** 32 * rate
    n = 4096 * M
    u = _tone(n, rate, fc + delta, amp=100.0 / 2 ** L)
    y = cm.channel(u, h, M, inc, L, P).astype(np.int64) - 128
    yc = y[0::2] + 1j * y[1::2]
    ideal = _ideal(u, h, M, inc, L)
    settle = len(h) // M + 1
    err = np.abs(yc[settle:].real - ideal[settle:].real).max(), np.abs(yc[settle:].imag - ideal[settle:].imag).max()
    assert max(err) <= 1.0, err
    # and the tone really sits at delta: the output's phase advances by 2 pi delta / 256 kS/s per sample
    rot = np.angle(np.sum(yc[settle + 1:] * np.conj(yc[settle:-1])))
    assert abs(rot - 2 * np.pi * delta / FS_OUT) < 1e-2


@pytest.mark.parametrize("M", [4, 8, 16])
@pytest.mark.parametrize("side", [-1, 1])
def test_tone_170_khz_off_the_channel_is_45_db_down(capi, M, side):
    """Measured on the int16 stage a (the 8-bit output cannot resolve it): the aliased out-of-band tone's FFT bin against
    the bin of an in-band tone of the same amplitude.  Every frequency sits on a bin of the 4096-point FFT."""
    rate = FS_OUT * M
    P = capi.channelizer_phasor_table()
    h = capi.channelizer_default_taps(M)
    fc = 62.5 * 3200 * (1 if M != 4 else -1)          # 200 kHz (-200 kHz), a bin
    inc = capi.phase_inc(fc, rate)
    assert np.int32(np.uint32(inc)).item() / 2.0 ** 32 * rate == fc
    N = 4096
    peaks = []
    for delta in (10e3, side * 170e3):
        u = _tone((N + 64) * M, rate, fc + delta)
        ar, ai = cm.channel(u, h, M, inc, 0, P, stage_a=True)
        a = (ar + 1j * ai)[64:]
        spec = np.abs(np.fft.fft(a))
        f_alias = ((fc + delta) % FS_OUT)
        peaks.append(spec[int(round(f_alias / (FS_OUT / N))) % N])
    assert 20 * np.log10(peaks[0] / peaks[1]) >= 45.0, peaks


def test_model_saturates_on_both_rails(capi):
    """Full-scale DC with L = 8 drives both saturations; L = 0 is unity gain (full scale in, full scale out)."""
    P = capi.channelizer_phasor_table()
    h = capi.channelizer_default_taps(8)
    hi = np.full(2 * 8 * 512, 255, np.uint8)
    lo = np.zeros(2 * 8 * 512, np.uint8)
    settle = 2 * (len(h) // 8 + 1)
    assert (cm.channel(hi, h, 8, 0, 8, P)[settle:] == 255).all()
    assert (cm.channel(lo, h, 8, 0, 8, P)[settle:] == 0).all()
    y = cm.channel(hi, h, 8, 0, 0, P)[settle:].astype(int) - 128
    assert (np.abs(y - 127) <= 1).all()


def test_isa_lint_of_the_channelizer_kernel():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_chan.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
