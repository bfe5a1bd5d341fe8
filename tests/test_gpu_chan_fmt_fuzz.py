"""GPU (MI355X): the fixed-seed slice of tools/chan_fuzz.py's format cases - the channelizer on signed 8-bit and 16-bit
captures at random decimations, tap counts and scales, inputs of the format's dtype, sources (some without channels),
channel counts and call lengths (the long ones by iqd_channelizer_window_outputs of the format), with retuning, moving,
resets and the host and device forms between the calls, every checked channel of every call byte for byte against
tests/chan_fmt_model.py.  tests/test_chan_fmt_fuzz_host.py holds the slice to the model's defects and to the edges it must
reach.  Bound by a case count: the same cases on every machine.  One test per format (each draws the whole slice and runs
its own cases); on an MI355X the S8 half takes 0.6 s and the S16 half 0.2 s."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# what tests/test_chan_fmt_fuzz_host.py finds the slice to run, per format (its COUNTS)
COUNTS = {"s8": {"fmt cases": 22, "fmt device calls": 50, "fmt host calls": 35, "fmt ops": 35},
          "s16": {"fmt cases": 14, "fmt device calls": 30, "fmt host calls": 35, "fmt ops": 27}}


@pytest.mark.parametrize("fmt", ["s8", "s16"])
def test_random_format_cases_match_the_model(fmt):
    import chan_fuzz
    ctx = chan_fuzz.Context()
    seed, n = chan_fuzz.SLICES["fmt"]
    assert n == 36
    rng = np.random.default_rng(seed)
    for case in range(n):
        bad = chan_fuzz.fmt_case(rng, ctx, only=fmt)
        assert bad is None, (seed, case, bad)
    print(ctx.stats)
    for k, v in COUNTS[fmt].items():
        assert ctx.stats.get(k, 0) >= v, (k, ctx.stats)
    ctx.close()
