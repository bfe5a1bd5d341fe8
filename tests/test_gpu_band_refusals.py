"""GPU (MI355X): the refusals of the five band objects - status and iqd_last_error text of every one, and which wins where two
apply - equal to tests/golden/band_refusals.json byte for byte.  The table is tests/band_refusals.py's; the golden file is what
the library gave before its host code was folded onto csrc/iqd_band_host.h.  A refused call queues and counts nothing; a valid
run_device afterwards counts its one launch."""
import json
import os

import pytest

from tests import band_refusals as br

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "band_refusals.json")


@pytest.fixture(scope="module")
def got():
    from rtlsdrdiags_amd import capi
    return br.collect(capi)


def test_every_refusal_is_the_recorded_one(got):
    with open(GOLDEN) as f:
        text = f.read()
    want, table = json.loads(text), got["table"]
    assert sorted(table) == sorted(want)
    wrong = {k: (table[k], want[k]) for k in want if table[k] != want[k]}
    assert not wrong, wrong
    assert br.dump(table) == text


def test_refusals_count_nothing_and_a_valid_call_one_launch(got):
    assert got["moved"] == (0, 0)
    assert got["valid"] == {name: 1 for name in br.RUNS}
