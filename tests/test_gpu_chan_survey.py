"""GPU (MI355X): the channelizer's band survey (include/iqdemod.h: "Band survey") exactly equal to the numpy model
(tests/chan_survey_model.py) on the inputs of tests/chan_survey_cases.py (which tests/test_chan_survey_host.py holds to the
mutation proof), equal to the magnitudes iqd_accept_wideband reports for real channels on the same grid, without effect on
the channelizer's state or on the regular channels, its refusals, and through the iqdemod_wide tool.  No tolerance
anywhere."""
import os
import subprocess

import numpy as np
import pytest

from tests import chan_frac_cases as fc
from tests import chan_frac_model as fm
from tests import chan_model as cm
from tests import chan_survey_cases as sc
from tests import chan_survey_model as sm

pytestmark = pytest.mark.gpu
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
    return {c.name: c for c in sc.cases(capi)}


def _want(c, P, oracle, wide=None, m_first=None):
    wide = c.wide if wide is None else wide
    return sm.survey(wide, c.h, c.M, c.Q, c.inc, c.shift, P, c.block_out, c.m_first if m_first is None else m_first,
                     c.n_out, c.window, oracle)


def _channelizer(capi, c, n_channels=1):
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, c.M, n_channels, n_sources=c.n_src, taps=c.taps, decimation_den=c.Q)
    return eng, z


@pytest.mark.parametrize("name", sc.NAMES)
def test_equal_to_the_model(capi, P, oracle, cases, name):
    """After `pre` units were run (the history and the sample count a survey reads), the survey of the next call; the
    host form and the device form; then, after a reset, the same bytes surveyed as a first call: the points survive."""
    c = cases[name]
    want = _want(c, P, oracle)
    eng, z = _channelizer(capi, c)
    z.set_survey(phase_inc=c.inc, gain_shift=c.shift)
    if c.pre:
        z.run(c.before)
    got = z.survey(c.call, c.block_bytes)
    assert got.shape == want.shape and got.dtype == np.uint32
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:8], got[tuple(bad[0])], want[tuple(bad[0])])
    call = np.ascontiguousarray(c.call)
    d_in, d_mag = eng.dev_alloc(call.nbytes), eng.dev_alloc(want.nbytes)
    eng.dev_upload(d_in, call)
    z.survey_device(d_in, call.shape[1], c.block_bytes, d_mag)
    eng.synchronize()
    assert np.array_equal(eng.dev_download(d_mag, want.nbytes, np.uint32).reshape(want.shape), want)
    eng.dev_free(d_in)
    eng.dev_free(d_mag)
    if c.pre:
        z.reset()
        assert np.array_equal(z.survey(c.call, c.block_bytes), _want(c, P, oracle, wide=c.call, m_first=0))
    z.close()
    eng.close()


@pytest.mark.parametrize("M,Q,units,block_bytes", [(8, 1, 32, 256), (8, 1, 32, 2048), (75, 8, 4, 256), (5, 2, 16, 1024)])
def test_equal_to_the_magnitudes_of_accept_wideband(capi, M, Q, units, block_bytes):
    """the same grid as real channels on every source, an engine whose block is block_bytes: its magnitude[]"""
    rng = np.random.default_rng(40 + M)
    n_src, n_pts = 2, 12
    wide = np.stack([fc.stream(rng, 2 * units * 64 * M, "rails" if s == 0 else "random") for s in range(n_src)])
    inc = rng.integers(0, 2 ** 32, n_pts).astype(np.uint64)
    shift = rng.integers(0, 9, n_pts).astype(np.uint8)
    eng = capi.Engine(n_src * n_pts, block_bytes=block_bytes)
    z = capi.Channelizer(eng, M, n_src * n_pts, n_sources=n_src, decimation_den=Q)
    z.set_channels(0, source=np.repeat(np.arange(n_src), n_pts), phase_inc=np.tile(inc, n_src), gain_shift=np.tile(shift, n_src))
    z.set_survey(phase_inc=inc, gain_shift=shift)
    half = units * 64 * M
    for part in (wide[:, :half], wide[:, half:]):                       # the second call: real history on both paths
        got = z.survey(part, block_bytes)
        _, _, mag, _ = eng.accept_wideband(z, part)
        assert got.shape == (n_src, mag.shape[1], n_pts) and mag.shape[1] == units * 64 * Q // block_bytes
        assert np.array_equal(got, mag.reshape(n_src, n_pts, -1).transpose(0, 2, 1))
        assert got.max() > 0
    z.close()
    eng.close()


@pytest.mark.parametrize("name", ["M8-64", "75/8-tail"])
def test_a_survey_touches_nothing_and_regular_channels_do_not_touch_it(capi, P, oracle, cases, name):
    """survey(x) twice gives the same array; run(x) afterwards equals run(x) of a channelizer that never surveyed, and
    the model's rows; the regular channels configured alongside change neither."""
    c = cases[name]
    rng = np.random.default_rng(7)
    n_ch = 20
    src, inc, shift = fc.channel_set(rng, n_ch, c.n_src)
    eng = capi.Engine(1)
    za = capi.Channelizer(eng, c.M, n_ch, n_sources=c.n_src, taps=c.taps, decimation_den=c.Q)
    zb = capi.Channelizer(eng, c.M, n_ch, n_sources=c.n_src, taps=c.taps, decimation_den=c.Q)
    for z in (za, zb):
        z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    za.set_survey(phase_inc=c.inc, gain_shift=c.shift)
    want = _want(c, P, oracle)
    first_a, first_b = za.run(c.before), zb.run(c.before)
    assert np.array_equal(first_a, first_b)
    one = za.survey(c.call, c.block_bytes)
    two = za.survey(c.call, c.block_bytes)
    assert np.array_equal(one, two) and np.array_equal(one, want)
    ra, rb = za.run(c.call), zb.run(c.call)
    assert np.array_equal(ra, rb)
    if c.Q == 1:
        rows = np.stack([cm.channel(c.wide[s], c.h, c.M, int(d), int(L), P) for s, d, L in zip(src, inc, shift)])
    else:
        rows = fm.channelize(c.wide, c.h, c.M, c.Q, src, inc, shift, P)
    assert np.array_equal(np.concatenate([first_a, ra], axis=1), rows)
    za.set_survey(phase_inc=[])                                          # cleared: nothing to survey
    with pytest.raises(capi.IqdError) as ei:
        za.survey(c.call, c.block_bytes)
    assert ei.value.status == -1
    for z in (za, zb):
        z.close()
    eng.close()


def test_refusals_queue_nothing(capi, P, oracle, cases):
    c = cases["M8-64"]
    eng, z = _channelizer(capi, c, n_channels=2)
    L = capi._lib()

    def refused(fn, *a, **k):
        with pytest.raises(capi.IqdError) as ei:
            fn(*a, **k)
        assert ei.value.status == -1, (fn, a)

    refused(z.survey, c.call, c.block_bytes)                             # no points set
    refused(z.set_survey, phase_inc=np.zeros(4097, np.uint32))
    refused(z.set_survey, phase_inc=[1, 2], gain_shift=[0, 9])
    assert L.iqd_channelizer_set_survey(z._h, 3, None, None) == -1       # points without increments
    refused(z.survey, c.call, c.block_bytes)                             # (the refused settings set nothing)
    z.set_survey(phase_inc=c.inc, gain_shift=c.shift)
    z.run(c.before)
    z.follow_scanner(True, 0, 1)
    refused(z.survey, c.call, c.block_bytes)                             # a channel follows its scanner
    z.follow_scanner(False, 0, 1)
    for n_bytes in (0, 64, 64 * 8 + 64, 64 * 4):                         # not a positive multiple of 64 M
        refused(z.survey, np.zeros((c.n_src, n_bytes), np.uint8), 64)
    row = c.call.shape[1] // c.M                                         # 2240 row bytes
    for bb in (0, 32, 96, 100, 128, 2 * row, 2 ** 32 - 64):              # not a multiple of 64, or no divisor of the row
        assert bb == 0 or bb % 64 or row % bb
        refused(z.survey, c.call, bb)
    call = np.ascontiguousarray(c.call)
    d_in, d_mag = eng.dev_alloc(call.nbytes + 16), eng.dev_alloc(4 * c.n_src * (row // 64) * c.n_pts + 16)
    eng.dev_upload(d_in, call)
    for wd, md in ((0, d_mag), (d_in, 0), (d_in + 8, d_mag), (d_in, d_mag + 4)):     # NULL, not 16-byte aligned
        refused(z.survey_device, wd, call.shape[1], 64, md)
    eng.dev_free(d_in)
    eng.dev_free(d_mag)
    # a block over 2^24 bytes (it divides the row and is a multiple of 64)
    e2 = capi.Engine(1)
    z2 = capi.Channelizer(e2, 2, 1)
    z2.set_survey(phase_inc=[5])
    refused(z2.survey, np.zeros((1, 2 ** 26), np.uint8), 2 ** 25)
    z2.close()
    e2.close()
    # fractional: multiples of 256 only
    f = cases["5/2-256"]
    e3, z3 = _channelizer(capi, f)
    z3.set_survey(phase_inc=f.inc, gain_shift=f.shift)
    for bb in (64, 128, 384):
        assert (f.call.shape[1] * f.Q // f.M) % bb == 0
        refused(z3.survey, f.call, bb)
    z3.run(f.before)
    assert np.array_equal(z3.survey(f.call, f.block_bytes), _want(f, P, oracle))
    z3.close()
    e3.close()
    # nothing was queued and nothing moved: the valid call gives the model's numbers
    assert np.array_equal(z.survey(c.call, c.block_bytes), _want(c, P, oracle))
    z.close()
    eng.close()


STATIONS = [  # offsets from the capture's centre
    {"offset": -700e3, "kind": "fm", "amplitude": 25.0, "tone": 1000.0, "mode": "fm"},
    {"offset": 250e3, "kind": "am", "amplitude": 40.0, "tone": 700.0, "mode": "am"},
    {"offset": -150e3, "kind": "wbfm", "amplitude": 15.0, "tone": 1500.0, "mode": "wbfm"},
]


@pytest.mark.parametrize("rate,M,Q,demod", [(2048000, 8, 1, False), (2400000, 75, 8, True)])
def test_iqdemod_wide_survey_log_equals_the_python_path(capi, tmp_path, rate, M, Q, demod):
    """survey=first,step,count: every accept (calls of 2 engine blocks, then the capture's last, short block) is surveyed
    before it is run; without offsets= nothing is demodulated and no PCM file appears."""
    from rtlsdrdiags_amd import synth
    block = 32768 * M // Q                                              # wide bytes of one engine block
    n_bytes = 2 * block + block // 2
    wide = synth.wideband(n_bytes // 2, float(rate), STATIONS, seed=21)
    cap, log = tmp_path / "cap.iq", tmp_path / "survey.log"
    wide.tofile(cap)
    first, step, count, shift = -900000, 50000, 37, 2
    offs = [first + step * p for p in range(count)]
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_wide")
    args = [tool, "in=%s" % cap, "rate=%d" % rate, "blocks=2", "survey=%d,%d,%d" % (first, step, count),
            "surveyshift=%d" % shift, "surveylog=%s" % log]
    chans = [st["offset"] + 64e3 for st in STATIONS]
    if demod:
        args += ["offsets=" + ",".join("%d" % o for o in chans), "modes=2", "out=%s" % (tmp_path / "pcm_%d.s16")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("pcm_")) == \
        (["pcm_%d.s16" % c for c in range(len(chans))] if demod else [])
    n = len(chans) if demod else 1
    eng = capi.Engine(n)
    z = capi.Channelizer(eng, M, n, decimation_den=Q)
    if demod:
        z.set_channels(0, source=[0] * n, offset_hz=chans, fs=float(rate))
        eng.set_mode("fm")
    z.set_survey(offset_hz=offs, fs=float(rate), gain_shift=shift)
    want, blk = [], 0
    for piece, bb in ((wide[:2 * block], 32768), (wide[2 * block:], 16384)):
        mag = z.survey(piece, bb)[0]
        for b in range(mag.shape[0]):
            want += ["%d %d %d %d" % (blk + b, offs[p], mag[b, p], capi.magnitude_dbfs(mag[b, p])) for p in range(count)]
        blk += mag.shape[0]
        if demod:
            eng.accept_wideband(z, piece)
        else:
            z.run(piece)
    assert blk == 3 and open(log).read().splitlines() == want
    mags = np.array([int(line.split()[2]) for line in want[:count]])
    # the strongest station (250 kHz) stands out on the grid: the first block's maximum lies on a point that has it in
    # its passband (+-100 kHz)
    assert abs(offs[int(np.argmax(mags))] - 250000) <= 100000
    z.close()
    eng.close()


def test_iqdemod_wide_refuses_survey_with_scan(tmp_path):
    """a survey is refused while a channel follows its scanner: the tool says so before it opens a device"""
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_wide")
    cap = tmp_path / "cap.iq"
    np.zeros(64, np.uint8).tofile(cap)
    r = subprocess.run([tool, "in=%s" % cap, "rate=2048000", "offsets=0", "modes=2", "out=%s" % (tmp_path / "p_%d.s16"),
                        "scan=162400000,162500000,25000", "survey=0,12500,3", "surveylog=%s" % (tmp_path / "s.log")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "survey= cannot be combined with scan=" in r.stderr, r.stderr
