"""GPU (MI355X): a fixed-seed slice of tools/chan_fuzz.py's gain cases - gain-following and fixed channels of one
channelizer (iqd_channelizer_follow_gain) with drawn block sizes, AGC settings, manual gains and following flags, every row,
PCM sample, magnitude, flag and gain-trace entry against tests/chan_gain_model.py on oracle chains.  Bound by a case count:
the same cases on every machine."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_random_gain_cases_match_the_model(oracle):
    import chan_fuzz
    ctx = chan_fuzz.Context(oracle)
    seed, n = chan_fuzz.SLICES["gain"]
    assert n == 24
    rng = np.random.default_rng(seed)
    for case in range(n):
        bad = chan_fuzz.gain_case(rng, ctx)
        assert bad is None, (seed, case, bad)
    print(ctx.stats)
    st = ctx.stats
    assert st.get("gain blocks", 0) >= 3 * n and st.get("gain changes", 0) > n and st.get("blocks above 46 dB", 0) > 0, st
    assert st.get("follow toggles", 0) > 0 and st.get("manual gains", 0) > 0 and st.get("short blocks", 0) > 0, st
    ctx.close()
