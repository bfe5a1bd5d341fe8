"""GPU (MI355X): an engine closed before what hangs off it.  Engine.close() destroys its children first, so a Resampler, a
Filter and a Channelizer closed after their engine have nothing left to do: their results are those of the same objects
closed in the proper order, children first, and the late closes return."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def run_and_close(capi, children_first):
    rng = np.random.default_rng(11)
    x = rng.normal(0, 500, 256).astype(np.float32)
    wide = rng.integers(0, 256, 256, dtype=np.uint8)
    h = rng.normal(0, 0.2, 8).astype(np.float32)
    eng = capi.Engine(1)
    children = capi.Resampler(eng, "decimate_f32", h, 2), capi.Filter(eng, "fir_f32", h), capi.Channelizer(eng, 4, 1)
    out = children[0].run(x), children[1].run(x), children[2].run(wide)
    if children_first:
        for c in children:
            c.close()
    eng.close()
    for c in children:
        c.close()
        assert not c._h
    return out


def test_children_closed_after_their_engine():
    from rtlsdrdiags_amd import capi
    want = run_and_close(capi, children_first=True)
    got = run_and_close(capi, children_first=False)
    assert [o.shape for o in want] == [(1, 128), (1, 256), (1, 64)] and all(o.any() for o in want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint8), w.view(np.uint8))
