"""GPU (MI355X): the stand-alone filters (iqd_filter_*: Decimator_int16, FirFilter_int16, FirFilter, IirFilter) bit for bit
against the model of tests/filter_model.py on the inputs of tests/filter_cases.py (which tests/test_filter_host.py proves
against the oracle, the reference and the model's defects), against the reference's golden vectors, the oracle, the
existing resampler, and the command-line tool.  Every comparison is equality of bit patterns.

Left out: decimate_i16 with the audio40 taps on an FM channel's int16 detector stream against the engine's own PCM - the
C ABI hands out no stage input of a chain (iqd_demod_accept goes from IQ bytes to PCM), so the stream is not reachable."""
import os
import subprocess

import numpy as np
import pytest

import filter_cases as fc
import filter_model as fm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fc.load()
STD = [0, 1, 2, 5, 700, 701, 1999]


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def eng(capi):
    e = capi.Engine(1)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def run_device_cut(eng, f, x, cuts, skew=True):
    """the device form, call by call; with skew, every other call's buffers start one element off a 16-byte boundary"""
    n_ch, item = x.shape[0], x.dtype.itemsize
    cap = n_ch * max(1, max(b - a for a, b in zip(cuts[:-1], cuts[1:]))) * item + 64
    d_in, d_out = eng.dev_alloc(cap), eng.dev_alloc(cap)
    outs = []
    try:
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            off = item if (skew and i % 2) else 0
            n_out = f.out_count(b - a)
            if b > a:
                eng.dev_upload(d_in + off, np.ascontiguousarray(x[:, a:b]))
            f.run_device(d_in + off, b - a, d_out + off)
            if n_out:
                outs.append(eng.dev_download(d_out + off, n_ch * n_out * item, x.dtype).reshape(n_ch, n_out))
        eng.synchronize()
    finally:
        eng.dev_free(d_in)
        eng.dev_free(d_out)
    return np.concatenate(outs, axis=1) if outs else np.zeros((n_ch, 0), x.dtype)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_equals_the_model(capi, eng, case):
    c = case
    want = fm.run(c.kind, c.num, c.den, c.factor, c.x, c.cuts)
    f = capi.Filter(eng, c.kind, c.num, c.den, c.factor, c.x.shape[0])
    try:
        got = f.run(c.x)                                     # the host form, one long call
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), np.argwhere(got != want)[:5]
        f.reset()
        got = run_device_cut(eng, f, c.x, c.cuts)            # the device form, cut as the case says
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), np.argwhere(got != want)[:5]
    finally:
        f.close()


Q15_GOLDEN = [("wbfm_pre", 1), ("wbfm_d1", 4), ("wbfm_d2", 4), ("audio40", 2), ("fm_tuner", 4), ("am_s1", 4), ("am_s2", 4),
              ("am_s3", 2), ("ssb_delay", 1), ("ssb_hilbert", 1)]


def uneven(f, x):
    cuts = [c for c in STD if c < len(x)] + [len(x)]
    return np.concatenate([f.run(x[a:b])[0] for a, b in zip(cuts[:-1], cuts[1:])])


@pytest.mark.parametrize("name,factor", Q15_GOLDEN)
def test_q15_goldens_in_uneven_calls(capi, eng, oracle, golden, name, factor):
    g = golden["primitives"]
    h = oracle.taps_f32(name)
    kinds = ["decimate_i16"] + (["fir_i16"] if factor == 1 else [])
    for kind in kinds:
        f = capi.Filter(eng, kind, h, None, factor)
        for src, dst in (("x16", "y16_"), ("xsat", "ysat_")):
            got = uneven(f, g[src])
            assert got.dtype == np.int16 and np.array_equal(got, g[dst + name]), (name, kind, src)
            f.reset()
            assert np.array_equal(f.run(g[src])[0], g[dst + name]), (name, kind, src, "after reset")
            f.reset()
        f.close()


def test_float_goldens_in_uneven_calls(capi, eng, golden):
    g = golden["primitives"]
    impulse = np.zeros(16, np.float32)
    impulse[0] = 1
    step = np.ones(32, np.float32)
    todo = [("fir_f32", [1, 2, 3, 4, 1, 1, 1, 8], None, impulse, "demo_fir_impulse"),
            ("iir_f32", [1.0], [0.5], step, "demo_iir_half_step"),
            ("iir_f32", [1.0, -1.0], [-0.95], step, "demo_dcblock_step"),
            ("iir_f32", [0.0253863, 0.0253863], [-0.9492274], g["xf"], "deemph_xf"),     # the chains' de-emphasis
            ("iir_f32", [1.0, -1.0], [-0.95], g["xf"], "dcblock_xf")]                    # ... and DC blocker
    for kind, num, den, x, key in todo:
        f = capi.Filter(eng, kind, num, den)
        got = uneven(f, x)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(g[key])), key
        f.reset()
        assert np.array_equal(bits(f.run(x)[0]), bits(g[key])), (key, "after reset")
        f.close()


def test_many_channels_against_the_oracle(capi, eng, oracle):
    rng = np.random.default_rng(3)
    n_ch, n = 300, 4096
    xf = rng.normal(0, 500, (n_ch, n)).astype(np.float32)
    x16 = rng.integers(-32768, 32768, (n_ch, n)).astype(np.int16)
    h48 = rng.normal(0, 0.2, 48).astype(np.float32)
    h40 = rng.uniform(-0.5, 0.5, 40).astype(np.float32)
    b, a = fc.stable_iir(rng, 3, 2)
    fir = capi.Filter(eng, "fir_f32", h48, None, 1, n_ch)
    dec = capi.Filter(eng, "decimate_i16", h40, None, 5, n_ch)
    iir = capi.Filter(eng, "iir_f32", b, a, 1, n_ch)
    y = np.concatenate([fir.run(xf[:, :1001]), fir.run(xf[:, 1001:])], axis=1)
    d = np.concatenate([dec.run(x16[:, :1001]), dec.run(x16[:, 1001:])], axis=1)
    r = np.concatenate([iir.run(xf[:, :333]), iir.run(xf[:, 333:])], axis=1)
    for c in range(0, n_ch, 37):
        assert np.array_equal(bits(y[c]), bits(oracle.decimate_f32(h48, 1, xf[c]))), c
        assert np.array_equal(d[c], oracle.decimate_q15(h40, 5, x16[c])), c
        assert np.array_equal(bits(r[c]), bits(oracle.iir_f32(b, a, xf[c]))), c
    for f in (fir, dec, iir):
        f.close()


def test_equivalences_that_do_not_rest_on_the_model(capi, eng):
    rng = np.random.default_rng(4)
    n_ch, n = 7, 3001
    xf = rng.normal(0, 500, (n_ch, n)).astype(np.float32)
    h = rng.normal(0, 0.2, 33).astype(np.float32)
    fir, dec = capi.Filter(eng, "fir_f32", h, None, 1, n_ch), capi.Resampler(eng, "decimate_f32", h, 1, n_ch)
    a = np.concatenate([fir.run(xf[:, :700]), fir.run(xf[:, 700:])], axis=1)
    b = np.concatenate([dec.run(xf[:, :1999]), dec.run(xf[:, 1999:])], axis=1)
    assert np.array_equal(bits(a), bits(b))                  # FirFilter = the float Decimator at factor 1
    x16 = np.where(rng.random((n_ch, n)) < 0.3, 32767, rng.integers(-32768, 32768, (n_ch, n))).astype(np.int16)
    hq = rng.uniform(-0.9, 0.9, 24).astype(np.float32)
    f1, d1 = capi.Filter(eng, "fir_i16", hq, None, 1, n_ch), capi.Filter(eng, "decimate_i16", hq, None, 1, n_ch)
    a = np.concatenate([f1.run(x16[:, :5]), f1.run(x16[:, 5:])], axis=1)
    assert np.array_equal(a, d1.run(x16))                    # FirFilter_int16 = Decimator_int16 at factor 1
    for f in (fir, dec, f1, d1):
        f.close()


def test_refusals_queue_nothing(capi, eng):
    rng = np.random.default_rng(6)
    h = rng.uniform(-0.5, 0.5, 9).astype(np.float32)
    x = rng.integers(-32768, 32768, (2, 500)).astype(np.int16)
    want = fm.run("decimate_i16", h, None, 3, x)
    L = eng._L
    import ctypes as C

    def create(kind, num, n_num, den, n_den, factor, n_ch, out=True):
        hnd = C.c_void_p()
        p = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(C.c_void_p)
        rc = L.iqd_filter_create(eng._h, kind, p(num), n_num, p(den), n_den, factor, n_ch, C.byref(hnd) if out else None)
        return rc, L.iqd_last_error(eng._h).decode()

    one = np.ones(2000, np.float32)
    bad = [((4, one, 8, None, 0, 1, 1), "kind"), ((-1, one, 8, None, 0, 1, 1), "kind"),
           ((0, None, 8, None, 0, 1, 1), "num"), ((0, one, 0, None, 0, 1, 1), "n_num"), ((0, one, 1025, None, 0, 1, 1), "n_num"),
           ((0, one, 8, None, 0, 0, 1), "factor"), ((0, one, 8, None, 0, 65, 1), "factor"), ((1, one, 8, None, 0, 2, 1), "factor"),
           ((2, one, 8, None, 0, 2, 1), "factor"), ((3, one, 2, one, 1, 2, 1), "factor"),
           ((0, one, 8, one, 0, 1, 1), "den"), ((0, one, 8, None, 1, 1, 1), "n_den"), ((2, one, 8, one, 1, 1, 1), "n_den"),
           ((3, one, 2, None, 1, 1, 1), "den"), ((3, one, 2, one, 0, 1, 1), "n_den"), ((3, one, 2, one, 65, 1, 1), "n_den"),
           ((3, one, 65, one, 1, 1, 1), "n_num"), ((0, one, 8, None, 0, 1, 0), "n_channels")]
    f = capi.Filter(eng, "decimate_i16", h, None, 3, 2)
    first = f.run(x[:, :200])
    launches = eng.stats()["device_launches"]
    for args, word in bad:
        rc, msg = create(*args)
        assert rc == -1 and word in msg, (args[0], args[2:], msg)
    assert create(0, one, 8, None, 0, 1, 1, out=False)[0] == -1
    d = eng.dev_alloc(4096)
    for args in [(None, 10, d), (d, 10, None), (d, 2 ** 31, d)]:
        with pytest.raises(capi.IqdError) as ei:
            f.run_device(*args)
        assert ei.value.status == -1
    assert L.iqd_filter_run(f._h, None, 10, x.ctypes.data_as(C.c_void_p)) == -1
    f.run_device(d, 0, d)                                    # nothing to do is not an error and moves nothing
    eng.dev_free(d)
    assert eng.stats()["device_launches"] == launches       # nothing was queued
    rest = f.run(x[:, 200:])                                 # the stream stands where it stood
    assert np.array_equal(np.concatenate([first, rest], axis=1), want)
    assert eng.stats()["device_launches"] == launches + 1
    f.close()


def tool(args, stdin=None):
    exe = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_filter")
    r = subprocess.run([exe] + args, input=stdin, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def test_tool_against_the_python_path(capi, eng, tmp_path):
    rng = np.random.default_rng(8)
    h = rng.uniform(-0.9, 0.9, 24).astype(np.float32)
    np.savetxt(tmp_path / "h.txt", h, fmt="%.9g")
    x = np.where(rng.random((3, 5000)) < 0.3, -32768, rng.integers(-32768, 32768, (3, 5000))).astype(np.int16)
    f = capi.Filter(eng, "decimate_i16", h, None, 4, 3)
    want = f.run(x)
    f.close()
    out = tool(["kind=decimate_i16", "taps=%s" % (tmp_path / "h.txt"), "factor=4", "chunk=777"], x[0].tobytes())
    assert np.array_equal(np.frombuffer(out, np.int16), want[0])
    for c in range(3):
        x[c].tofile(tmp_path / ("x_%d.raw" % c))
    tool(["kind=decimate_i16", "taps=%s" % (tmp_path / "h.txt"), "factor=4", "channels=3", "in=%s" % (tmp_path / "x_%d.raw"),
          "out=%s" % (tmp_path / "y_%d.raw"), "chunk=1001"])
    for c in range(3):
        assert np.array_equal(np.fromfile(tmp_path / ("y_%d.raw" % c), np.int16), want[c]), c
    b, a = fc.stable_iir(rng, 3, 2)
    np.savetxt(tmp_path / "b.txt", b, fmt="%.9g")
    np.savetxt(tmp_path / "a.txt", a, fmt="%.9g")
    xf = rng.normal(0, 3000, (2, 3000)).astype(np.float32)
    f = capi.Filter(eng, "iir_f32", b, a, 1, 2)
    want = f.run(xf)
    f.close()
    out = tool(["kind=iir_f32", "taps=%s" % (tmp_path / "b.txt"), "den=%s" % (tmp_path / "a.txt"), "chunk=64"], xf[1].tobytes())
    assert np.array_equal(bits(np.frombuffer(out, np.float32)), bits(want[1]))
    for c in range(2):
        xf[c].tofile(tmp_path / ("xf_%d.raw" % c))
    tool(["kind=iir_f32", "taps=%s" % (tmp_path / "b.txt"), "den=%s" % (tmp_path / "a.txt"), "channels=2",
          "in=%s" % (tmp_path / "xf_%d.raw"), "out=%s" % (tmp_path / "yf_%d.raw")])
    for c in range(2):
        assert np.array_equal(bits(np.fromfile(tmp_path / ("yf_%d.raw" % c), np.float32)), bits(want[c])), c
