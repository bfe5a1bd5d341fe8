"""GPU (MI355X): a fixed-seed slice of tools/chan_fuzz.py's track cases - track-following and fixed channels of one
channelizer (iqd_channelizer_follow_tracks) with drawn decimations, taps, tables, block sizes, lags and call forms, every
row, PCM sample, magnitude and flag against tests/chan_track_model.py.  Bound by a case count: the same cases on every
machine."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_random_track_cases_match_the_model(oracle):
    import chan_fuzz
    ctx = chan_fuzz.Context(oracle)
    seed, n = chan_fuzz.SLICES["track"]
    assert n == 24
    rng = np.random.default_rng(seed)
    for case in range(n):
        bad = chan_fuzz.track_case(rng, ctx)
        assert bad is None, (seed, case, bad)
    print(ctx.stats)
    st = ctx.stats
    assert st.get("track cases", 0) == n and st.get("track blocks", 0) >= 3 * n, st
    assert 0 < st.get("live blocks", 0) < st.get("track blocks", 0), st
    assert st.get("large K cases", 0) > 0 and st.get("track toggles", 0) > 0, st
    ctx.close()
