"""GPU (MI355X): fixed-seed slices of tools/chan_fuzz.py - random decimations, tap counts and scales, inputs, sources,
channel counts, call lengths and operator steps between calls, every compared channel bit for bit against the model -
a slice of scanner-driven cases against the scan model on oracle chains, and the two fixed walker geometries.  The
slices are bound by case counts: the same cases on every machine (tests/test_chan_corpus_host.py shows on the CPU that
the plain slices expose every defect of tests/chan_mutants.py)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


@pytest.fixture(scope="module")
def ctx(oracle):
    import chan_fuzz
    c = chan_fuzz.Context(oracle)
    yield c
    c.close()


@pytest.mark.parametrize("slice_", [0, 1])
def test_random_plain_cases_match_the_model(ctx, slice_):
    import chan_fuzz
    seed, n = chan_fuzz.SLICES["plain"][slice_]
    assert n == 150
    rng = np.random.default_rng(seed)
    for case in range(n):
        bad = chan_fuzz.plain_case(rng, ctx)
        assert bad is None, (seed, case, bad)


def test_random_scan_cases_match_the_model(ctx):
    import chan_fuzz
    seed, n = chan_fuzz.SLICES["scan"]
    assert n == 40
    ctx.stats.clear()
    rng = np.random.default_rng(seed)
    for case in range(n):
        bad = chan_fuzz.scan_case(rng, ctx)
        assert bad is None, (seed, case, bad)
    # the slice met what it is there for: blocks out of band, squelches that opened and stayed shut, scanners that moved,
    # short blocks, the AGC, and channels that began or stopped following between calls
    st = ctx.stats
    print(st)
    for key in ("silent blocks", "open blocks", "closed blocks", "retunes", "short blocks", "agc blocks", "follow toggles",
                "scanner commands"):
        assert st.get(key, 0) >= 3, (key, st)
    assert st["silent blocks"] < st["blocks"] // 2, st


def test_walker_workgroups_of_three_tiles(ctx):
    """3 x (compute units) following tiles at 256-byte engine blocks: three tiles per workgroup, two waves per tile."""
    import chan_fuzz
    cus = chan_fuzz.compute_units()       # torch.cuda.get_device_properties(0).multi_processor_count
    assert cus >= 1
    bad = chan_fuzz.fixed_scan_case("waves3", ctx, cus=cus)
    assert bad is None, (cus, bad)


def test_walker_last_window_of_64_outputs(ctx):
    """M = 64, K = 1024 (windows of 192 outputs) at 2048-byte engine blocks: 1024 = 5 x 192 + 64."""
    import chan_fuzz
    assert chan_fuzz.t_max(64, 1024) == 192
    bad = chan_fuzz.fixed_scan_case("window64", ctx)
    assert bad is None, bad
