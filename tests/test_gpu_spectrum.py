"""GPU (MI355X): the band spectrum (include/iqdemod.h: "Band spectrum") exactly equal to the numpy model
(tests/spectrum_model.py) on the inputs of tests/spectrum_cases.py (which tests/test_spectrum_host.py holds to the mutation
proof), in host and device form, beside a channelizer on the same capture buffer, its refusals, through the
iqdemod_spectrum tool, and on a synthetic band of two stations.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import spectrum_cases as sc
from tests import spectrum_model as sm

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
def cases(P):
    return {c.name: c for c in sc.cases(P)}


@pytest.fixture(scope="module")
def wants(P, cases):
    """name -> the model's array, computed once and shared"""
    out = {}

    def get(name):
        if name not in out:
            c = cases[name]
            out[name] = sm.spectrum(c.wide, c.fmt, c.N, c.F, c.w(P), P)
            out[name].setflags(write=False)
        return out[name]
    return get


def _same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint32
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:8], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", sc.NAMES)
def test_equal_to_the_model(capi, cases, wants, name):
    """the host form; the device form; a second device call into the same buffers (no state from call to call)"""
    c, want = cases[name], wants(name)
    eng = capi.Engine(1)
    s = capi.Spectrum(eng, c.N, n_sources=c.n_src, window=c.window, sample_format=c.fmt)
    _same(s.run(c.wide, c.F), want)
    wide = np.ascontiguousarray(c.wide)
    d_in, d_out = eng.dev_alloc(wide.nbytes), eng.dev_alloc(want.nbytes)
    eng.dev_upload(d_in, wide.view(np.uint8))
    for _ in range(2):
        s.run_device(d_in, wide.shape[1], c.F, d_out)
        eng.synchronize()
        _same(eng.dev_download(d_out, want.nbytes, np.uint32).reshape(want.shape), want)
    assert np.array_equal(eng.dev_download(d_in, wide.nbytes), wide.view(np.uint8).ravel())      # the capture is only read
    eng.dev_free(d_in)
    eng.dev_free(d_out)
    s.close()
    eng.close()


def test_full_scale_on_the_constant_input(capi, cases, wants):
    c = cases["N1024-const-F32"]
    eng = capi.Engine(1)
    s = capi.Spectrum(eng, c.N)
    got = s.run(c.wide, c.F)
    p_fs = capi.spectrum_full_scale(c.N)
    assert got[0, 0, c.N // 2] == p_fs == 264225025 and c.F * p_fs > 2 ** 32
    assert capi.spectrum_dbfs(got[0, 0, c.N // 2], p_fs) == 0.0
    _same(got, wants(c.name))
    s.close()
    eng.close()


@pytest.mark.parametrize("name", ["N64-F32-random", "N2048-F2-s8"])
def test_beside_a_channelizer_on_the_same_capture_buffer(capi, cases, wants, name):
    """One engine, one device buffer: channelizer, spectrum, channelizer, spectrum.  The channelizer's rows are the same
    before and after (and what a channelizer that never met a spectrum gives), the spectrum is the model's both times."""
    c, want = cases[name], wants(name)
    M, n_ch = 8, 3
    wide = np.ascontiguousarray(c.wide)
    assert c.n_src == 1 and wide.shape[1] % (64 * M) == 0
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, M, n_ch, sample_format=c.fmt)
    z.set_channels(0, source=[0] * n_ch, phase_inc=[0, 123456789, 2 ** 32 - 987654321], gain_shift=[0, 3, 8])
    alone = z.run(wide)
    s = capi.Spectrum(eng, c.N, window=c.window, sample_format=c.fmt)
    d_in, d_rows, d_out = eng.dev_alloc(wide.nbytes), eng.dev_alloc(alone.nbytes), eng.dev_alloc(want.nbytes)
    eng.dev_upload(d_in, wide.view(np.uint8))
    for _ in range(2):
        z.reset()
        z.run_device(d_in, wide.shape[1], d_rows)
        s.run_device(d_in, wide.shape[1], c.F, d_out)
        eng.synchronize()
        assert np.array_equal(eng.dev_download(d_rows, alone.nbytes).reshape(alone.shape), alone)
        _same(eng.dev_download(d_out, want.nbytes, np.uint32).reshape(want.shape), want)
    for d in (d_in, d_rows, d_out):
        eng.dev_free(d)
    s.close()
    z.close()
    eng.close()


def test_refusals_queue_nothing(capi, cases, wants):
    c = cases["N64-F32-random"]
    want = wants(c.name)
    eng = capi.Engine(1)
    L = capi._lib()
    launches = eng.stats()["device_launches"]

    def refused(fn, *a, **k):
        with pytest.raises(capi.IqdError) as ei:
            fn(*a, **k)
        assert ei.value.status == -1, (fn, a)
        return str(ei.value)

    # create
    refused(capi.Spectrum, eng, 64, n_sources=0)
    for n in (0, 32, 96, 100, 4096, 2 ** 31):
        assert "n_bins" in refused(capi.Spectrum, eng, n)
    with pytest.raises(ValueError):
        capi.Spectrum(eng, 64, sample_format="f32")
    assert "IQD_WIDE_S16" in refused(capi.Spectrum, eng, 64, sample_format="s16")
    h = C.c_void_p()
    for cfg in (capi.SpectrumConfig(1, 64, None, 3), capi.SpectrumConfig(1, 64, None, 2 ** 32 - 1)):
        assert L.iqd_spectrum_create(eng._h, C.byref(cfg), C.byref(h)) == -1 and not h.value
        assert b"sample_format" in L.iqd_last_error(eng._h)
    for i in range(3):
        cfg = capi.SpectrumConfig(1, 64, None, 0)
        cfg.reserved[i] = 1
        assert L.iqd_spectrum_create(eng._h, C.byref(cfg), C.byref(h)) == -1 and not h.value
        assert b"reserved" in L.iqd_last_error(eng._h)
    cfg = capi.SpectrumConfig(1, 64, None, 0)
    assert L.iqd_spectrum_create(eng._h, None, C.byref(h)) == -1 and b"cfg" in L.iqd_last_error(eng._h)
    assert L.iqd_spectrum_create(eng._h, C.byref(cfg), None) == -1 and b"out" in L.iqd_last_error(eng._h)
    assert L.iqd_spectrum_create(None, C.byref(cfg), C.byref(h)) == -1
    w = np.zeros(64, np.int16)
    for bad in (32640, -32640):
        w[5] = bad
        assert "window[5]" in refused(capi.Spectrum, eng, 64, window=w)
    assert "window" in refused(capi.Spectrum, eng, 1024, window=np.full(1024, 8192, np.int16))
    with pytest.raises(ValueError):
        capi.Spectrum(eng, 64, window=np.zeros(63, np.int16))

    # run
    s = capi.Spectrum(eng, c.N, window=c.window, sample_format=c.fmt)
    s8 = capi.Spectrum(eng, c.N, sample_format="s8")
    with pytest.raises(TypeError):
        s.run(c.wide.view(np.int8), c.F)
    with pytest.raises(TypeError):
        s.run(c.wide.astype(np.int16), c.F)
    with pytest.raises(TypeError):
        s8.run(c.wide, c.F)
    s8.close()
    for F in (0, 2 ** 24 + 1, 2 ** 32 - 1):
        assert "frames_per_block" in refused(s.run, c.wide, F)
    one = 2 * c.N                                                         # bytes of one frame
    for n_bytes, F in ((0, 1), (one - 2, 1), (one + 16, 1), (3 * one, 2), (one, 2)):   # 0, or no multiple of 2 N F
        assert "bytes_per_source" in refused(s.run, np.zeros((1, n_bytes), np.uint8), F)
    wide = np.ascontiguousarray(c.wide)
    d_in, d_out = eng.dev_alloc(wide.nbytes + 16), eng.dev_alloc(want.nbytes + 16)
    eng.dev_upload(d_in, wide)
    for wd, pd, word in ((0, d_out, "wide"), (d_in, 0, "power"), (d_in + 8, d_out, "wide_dev"), (d_in, d_out + 4, "power_dev"),
                         (d_in + 1, d_out, "wide_dev")):
        assert word in refused(s.run_device, wd, wide.shape[1], c.F, pd)
    for n_bytes, F in ((0, c.F), (wide.shape[1] - one, c.F), (wide.shape[1], 0), (wide.shape[1], 2 ** 24 + 1)):
        refused(s.run_device, d_in, n_bytes, F, d_out)
    assert L.iqd_spectrum_run_device(None, C.c_void_p(d_in), wide.shape[1], c.F, C.c_void_p(d_out)) == -1
    # nothing was queued: no launch was counted, and the valid calls give the model's numbers
    assert eng.stats()["device_launches"] == launches
    s.run_device(d_in, wide.shape[1], c.F, d_out)
    eng.synchronize()
    _same(eng.dev_download(d_out, want.nbytes, np.uint32).reshape(want.shape), want)
    assert eng.stats()["device_launches"] == launches + 1
    _same(s.run(c.wide, c.F), want)
    eng.dev_free(d_in)
    eng.dev_free(d_out)
    s.close()
    eng.close()


STATIONS = [  # offsets from the capture's centre (2.048 MS/s), as tests/test_gpu_chan_fmt.py places them
    {"offset": -700e3, "kind": "fm", "amplitude": 25.0, "tone": 1000.0, "mode": "fm"},
    {"offset": 250e3, "kind": "am", "amplitude": 25.0, "tone": 700.0, "mode": "am"},
]
RATE = 2048000.0


@pytest.mark.parametrize("fmt", ["u8", "s8"])
def test_iqdemod_spectrum_equals_the_python_path(capi, tmp_path, fmt):
    """out= is the API's array byte for byte, log= one line per block and bin; a capture that ends inside a block ends
    with its last whole block and the rest is counted on stderr"""
    N, F, blocks, rest = 256, 3, 2, 2 * 256 + 10
    rng = np.random.default_rng(77)
    wide = rng.integers(0, 256, 2 * N * F * blocks + rest, dtype=np.uint8)
    ramp = (np.arange(N) * 100 - 3000).astype(np.int16)
    cap, out, log, wtxt = tmp_path / "cap.iq", tmp_path / "power.u32", tmp_path / "spectrum.txt", tmp_path / "w.txt"
    wide.tofile(cap)
    wtxt.write_text(", ".join(str(v) for v in ramp[:N // 2]) + "\n" + " ".join(str(v) for v in ramp[N // 2:]) + "\n")
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_spectrum")
    r = subprocess.run([tool, "in=%s" % cap, "rate=2048000", "bins=%d" % N, "frames=%d" % F, "format=" + fmt,
                        "window=%s" % wtxt, "out=%s" % out, "log=%s" % log], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "%d bytes" % rest in r.stderr
    whole = wide[:2 * N * F * blocks].reshape(1, -1)
    eng = capi.Engine(1)
    s = capi.Spectrum(eng, N, window=ramp, sample_format=fmt)
    want = s.run(whole if fmt == "u8" else whole.view(np.int8), F)
    s.close()
    eng.close()
    assert want.shape == (1, blocks, N) and want.max() > 0
    assert out.read_bytes() == want.astype("<u4").tobytes()
    p_fs = capi.spectrum_full_scale(N, ramp)
    lines = log.read_text().splitlines()
    assert len(lines) == blocks * N
    for b in range(blocks):
        for k in (0, 1, N // 2, N - 1):
            blk, off, p, db = lines[b * N + k].split()
            assert (int(blk), float(off), int(p)) == (b, (k - N // 2) * RATE / N, int(want[0, b, k]))
            assert abs(float(db) - capi.spectrum_dbfs(want[0, b, k], p_fs)) <= 0.006      # two decimals
    bad = subprocess.run([tool, "in=%s" % cap, "rate=2048000", "bins=100", "frames=1", "out=%s" % out], capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 1 and "n_bins" in bad.stderr


@pytest.mark.parametrize("fmt", ["u8", "s8"])
def test_two_stations_stand_where_they_were_put(capi, P, fmt):
    """synth.wideband's two stations through Spectrum against the model; the strongest bins are the stations'"""
    from rtlsdrdiags_amd import synth
    N, F, blocks = 1024, 8, 2
    u8 = synth.wideband(N * F * blocks, RATE, STATIONS, seed=31).reshape(1, -1)
    wide = u8 if fmt == "u8" else (u8 ^ 0x80).view(np.int8)
    eng = capi.Engine(1)
    s = capi.Spectrum(eng, N, sample_format=fmt)
    got = s.run(wide, F)
    s.close()
    eng.close()
    _same(got, sm.spectrum(wide, fmt, N, F, None, P))
    at = [N // 2 + int(round(st["offset"] / (RATE / N))) for st in STATIONS]     # bins 162 and 637
    for b in range(blocks):
        top = np.argsort(got[0, b])[-2:]
        assert all(min(abs(int(k) - a) for a in at) <= 3 for k in top), (top, at)
        db = capi.spectrum_dbfs(got[0, b], capi.spectrum_full_scale(N))
        assert db[at[1]] > -20 and np.median(db) < -45                           # a carrier of 25 / 127, noise of sigma 2
