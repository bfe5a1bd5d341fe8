"""GPU (MI355X): the fixed slices of tools/band_fuzz.py - seeded spectrum, detector, tracker and chained cases, every array
bit for bit against the models (tests/spectrum_model.py, tests/detect_model.py, tests/track_model.py), in host form and
device form.  The slices are bound by case counts: the same cases on every machine.  tests/test_band_fuzz_host.py shows on
the CPU that they expose every defect of the models and hold the structures the kernels branch on."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

CASES = {"spectrum": 60, "detect": 150, "track": 90, "chain": 16}


@pytest.fixture(scope="module")
def ctx():
    import band_fuzz
    c = band_fuzz.Context()
    yield c
    c.close()


def _slice(ctx, kind):
    import band_fuzz
    seed, n = band_fuzz.SLICES[kind]
    assert n == CASES[kind]
    fn = band_fuzz.KINDS[kind]
    for case in range(n):
        bad = fn(band_fuzz.case_rng(seed, case), ctx)
        assert bad is None, (seed, case, bad)


def test_random_spectrum_cases_match_the_model(ctx):
    _slice(ctx, "spectrum")


def test_random_detect_cases_match_the_model(ctx):
    _slice(ctx, "detect")


def test_random_track_cases_match_the_model(ctx):
    _slice(ctx, "track")


def test_random_chain_cases_match_the_models(ctx):
    """Spectrum, Detector and Tracker queued on one stream with one synchronise, in buffers the cases before left as they
    were; the slice opened and closed tracks (counted from the model)"""
    ctx.stats.clear()
    _slice(ctx, "chain")
    print(ctx.stats)
    assert ctx.stats["chain opened"] >= 3 and ctx.stats["chain closed"] >= 3, ctx.stats
