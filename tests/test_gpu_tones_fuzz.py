"""GPU tier: a fixed slice of tools/tones_fuzz.py (seed and count: its SLICE) - every case's counts, records, power rows and
states bit for bit against tests/tones_model.py.  tests/test_tones_fuzz_host.py holds the same cases to a list of structural
conditions without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tones_fuzz as tf                                # noqa: E402
from rtlsdrdiags_amd import capi                       # noqa: E402

pytestmark = pytest.mark.gpu
PARTS = 6


@pytest.fixture(scope="module")
def rig():
    eng = capi.Engine(n_channels=1)
    bufs = tf.Buffers(eng)
    yield capi.channelizer_phasor_table(), eng, bufs
    bufs.close()
    eng.close()


@pytest.mark.parametrize("part", range(PARTS))
def test_fixed_slice(rig, part):
    phasor, eng, bufs = rig
    seed, cases = tf.SLICE
    assert cases % PARTS == 0
    for i in range(part * cases // PARTS, (part + 1) * cases // PARTS):
        tf.run_case(tf.draw(seed, i, phasor), phasor, eng, bufs)
