"""GPU tier: a fixed slice of tools/fsk_fuzz.py (seed and count: its SLICE) - every case's counts, bit words, records, bytes and
states bit for bit against tests/fsk_model.py.  tests/test_fsk_fuzz_host.py holds the same cases to a list of structural
conditions without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fsk_fuzz as ff                                  # noqa: E402
from rtlsdrdiags_amd import capi                       # noqa: E402

pytestmark = pytest.mark.gpu
PARTS = 6


@pytest.fixture(scope="module")
def rig():
    eng = capi.Engine(n_channels=1)
    bufs = ff.Buffers(eng)
    yield capi.channelizer_phasor_table(), eng, bufs
    bufs.close()
    eng.close()


@pytest.mark.parametrize("part", range(PARTS))
def test_fixed_slice(rig, part):
    phasor, eng, bufs = rig
    seed, cases = ff.SLICE
    assert cases % PARTS == 0
    for i in range(part * cases // PARTS, (part + 1) * cases // PARTS):
        ff.run_case(ff.draw(seed, i, phasor), phasor, eng, bufs)
