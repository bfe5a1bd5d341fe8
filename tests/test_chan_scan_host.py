"""CPU tier for scanner-driven wideband channels (include/iqdemod.h: iqd_channelizer_follow_scanner): the host-only
tuning rule against Python integers, the model's teeth (tests/chan_scan_model.py) and the ISA lint of the walker."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import chan_model as cm
from tests import chan_scan_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


def test_tuning_matches_the_rule(capi):
    rng = np.random.default_rng(5)
    cases = []
    for M in (2, 3, 8, 64):
        fs = 256000 * M
        # Exact half-way cases cannot occur: o 2^32 + Fs/2 = 0 mod Fs needs o 2^32 = Fs/2 mod Fs, and Fs = 256000 M holds
        # at most 2^17 of 2.  The offsets whose quotient comes nearest to a rounding boundary stand in for them.
        near = sorted(range(-fs // 2, -fs // 2 + 20000),
                      key=lambda o: min(((o << 32) + fs // 2) % fs, fs - ((o << 32) + fs // 2) % fs))[:6]
        for r in (-1, 0, 1):
            for centre in (0, 1_700_000_000, 162_550_000):
                st = centre - 64000 * r
                cases += [(M, centre, st - fs // 2, r), (M, centre, st + fs // 2, r), (M, centre, st + fs // 2 - 1, r),
                          (M, centre, st - fs // 2 - 1, r), (M, centre, st, r)]
                for o in near:
                    cases += [(M, centre, st + o, r), (M, centre, st + o + fs // 2, r)]
                for _ in range(20):
                    cases.append((M, centre, st + int(rng.integers(-fs, fs)), r))
        cases += [(M, 0, f, -1) for f in (0, 1, 63999, 64000)]            # f < 64000 with r = -1: negative centre
        cases += [(M, 2 ** 64 - 1, 2 ** 64 - 1, 0), (M, 0, 2 ** 64 - 1, 1), (M, 2 ** 64 - 1, 0, -1)]
    n_in = 0
    for M, c, f, r in cases:
        if f < 0 or f >= 2 ** 64 or c < 0:
            continue
        want = sm.tuning(M, c, f, r)
        got = capi.channelizer_tuning(M, c, f, r)
        assert got == want, (M, c, f, r, got, want)
        n_in += want is not None
    assert n_in > 100
    fs = 256000 * 8
    assert capi.channelizer_tuning(8, 10 ** 9, 10 ** 9 - fs // 2 - 64000, 1) == 2 ** 31       # -Fs/2: in band
    assert capi.channelizer_tuning(8, 10 ** 9, 10 ** 9 + fs // 2 - 64000, 1) is None          # +Fs/2: out of band
    assert capi.channelizer_tuning(8, 0, 1, -1) == sm.tuning(8, 0, 1, -1) == ((-63999 << 32) + fs // 2) // fs % 2 ** 32
    for bad in ((1, 0, 0, 1), (65, 0, 0, 1), (8, 0, 0, 2), (8, 0, 0, -2)):   # an error, not "out of band"
        with pytest.raises(capi.IqdError):
            capi.channelizer_tuning(*bad)


def _scene(M, n_blocks, block_out, seed):
    """a source at 1.7 GHz with carriers keyed on for some blocks"""
    from rtlsdrdiags_amd import synth
    fs = 256000 * M
    spb = block_out * M
    stations = [
        {"offset": 200_000, "kind": "fm", "amplitude": 40.0, "on": [(3 * spb, 6 * spb)]},
        {"offset": -300_000, "kind": "am", "amplitude": 40.0, "on": [(1 * spb, 2 * spb), (5 * spb, 8 * spb)]},
    ]
    return synth.wideband(n_blocks * spb, fs, stations, seed=seed, sigma=1.0)


def _chain(threshold, scan=None):
    from oracle.bindings import Oracle
    c = Oracle().chain()
    c.set_mode("fm")
    c.set_squelch(threshold)
    if scan:
        c.scanner_set_parameters(*scan)
        c.scanner_start()
    return c


def test_model_has_teeth_and_reduces_to_plain_channelize(capi):
    M, bo, nb = 4, 2048, 10
    centre = 1_700_000_000
    wide = _scene(M, nb, bo, 3)
    h = capi.channelizer_default_taps(M)
    P = capi.channelizer_phasor_table()
    # a grid over the capture: stops on the keyed carriers while they are on, moves on when they go
    scan = (centre - 300_000 - 64000, centre + 200_000 - 64000, 100_000)
    a = sm.follow(_chain(-50, scan), wide, h, M, P, 0, centre, bo, nb)
    b = sm.follow(_chain(-50, scan), wide, h, M, P, 0, centre, bo, nb, late=True)
    assert len(set(a[4].tolist())) > 2                    # the scanner moved
    assert a[3].any() and not a[3].all()                  # and stopped on something
    assert not np.array_equal(a[0], b[0]) or not np.array_equal(a[4], b[4])
    # stopped scanner: the whole row is plain channelize at the tuning increment
    st = centre + 200_000 - 64000
    c2 = _chain(-30)
    c2.scanner_set_parameters(st, st, 0)
    c2.scanner_start()
    c2.scanner_stop()
    rows = sm.follow(c2, wide, h, M, P, 2, centre, bo, nb)[0]
    inc = sm.tuning(M, centre, st, 1)
    want = cm.channelize(wide[None], h, M, [0], [inc], [2], P)[0]
    assert np.array_equal(rows, want)


def test_isa_lint_of_the_walker():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_chan.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
    assert "chz_scan_kernel" in r.stdout or " 5 kernels" in last, last
