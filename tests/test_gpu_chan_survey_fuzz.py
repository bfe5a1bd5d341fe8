"""GPU (MI355X): a fixed-seed slice of tools/chan_fuzz.py's survey cases - plain and fractional cases with band surveys
(iqd_channelizer_survey*) drawn before their calls, every entry against tests/chan_survey_model.py, and the calls that
follow against the channelizer's models as ever (a survey that moved the state would show there).  Bound by a case count:
the same cases on every machine."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_random_survey_cases_match_the_model(oracle):
    import chan_fuzz
    ctx = chan_fuzz.Context(oracle)
    seed, n = chan_fuzz.SLICES["survey"]
    assert n == 40
    rng = np.random.default_rng(seed)
    for case in range(n):
        bad = chan_fuzz.survey_case(rng, ctx)
        assert bad is None, (seed, case, bad)
    print(ctx.stats)
    assert ctx.stats["surveys"] >= n and ctx.stats["survey blocks"] > 2 * ctx.stats["surveys"], ctx.stats
    ctx.close()
