"""GPU (MI355X): the refusals of the channelizer's host code - status and iqd_last_error text of every one, and which wins where
two apply - equal to tests/golden/chan_refusals.json byte for byte.  The table is tests/chan_refusals.py's; the golden file is
what the library gave before csrc/iqd_chan.cpp was cut into one file per concern.  A refused call moves nothing: the valid runs
before and after the table give the model's rows of the two captures concatenated."""
import json
import os

import numpy as np
import pytest

from tests import chan_refusals as cr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chan_refusals.json")


@pytest.fixture(scope="module")
def got():
    from rtlsdrdiags_amd import capi
    return cr.collect(capi)


def test_every_refusal_is_the_recorded_one(got):
    with open(GOLDEN) as f:
        text = f.read()
    want, table = json.loads(text), got["table"]
    assert sorted(table) == sorted(want)
    wrong = {k: (table[k], want[k]) for k in want if table[k] != want[k]}
    assert not wrong, wrong
    assert cr.dump(table) == text


@pytest.mark.parametrize("name", ["u8", "frac", "s8", "s16"])
def test_no_refused_call_moved_the_stream(got, name):
    rows, want = got["rows"][name], got["want"][name]
    assert rows.shape == want.shape and rows.shape[0] == cr.NCH
    assert np.array_equal(rows, want)
