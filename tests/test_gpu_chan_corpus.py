"""GPU (MI355X): the channelizer's directed edge corpus (tests/chan_corpus.py; tests/test_chan_corpus_host.py shows on
the CPU which defect each family exposes) through iqd_channelizer_run, bit for bit against the model: every case in one
call, again in its call cuts (shortest calls that carry the history across many of them), and in other tile slots."""
import numpy as np
import pytest

from tests import chan_corpus as cc
from tests import chan_model as cm

pytestmark = pytest.mark.gpu
FAMILIES = ("final_tie", "a_tie_1tap", "low_order", "sat16", "tap_edges", "general")


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def corpus(capi, P):
    return cc.cases(P, capi.channelizer_default_taps)


@pytest.fixture(scope="module")
def eng(capi):
    e = capi.Engine(1)
    yield e
    e.close()


def _differs(got, want):
    d = np.flatnonzero(got != want)
    return "%d bytes differ, first at byte %d (outputs %s): got %s, model %s" % (
        len(d), d[0], np.unique(d // 2)[:12].tolist(), got[d[:8]].tolist(), want[d[:8]].tolist())


@pytest.mark.parametrize("family", FAMILIES)
def test_one_call_and_the_call_cuts(capi, P, corpus, eng, family):
    cases = [c for c in corpus if c.family == family]
    assert cases
    for c in cases:
        want = cm.channel(c.wide, c.h, c.M, c.inc, c.L, P)
        z = capi.Channelizer(eng, c.M, 1, taps=c.h)
        z.set_channels(0, phase_inc=[c.inc], gain_shift=[c.L])
        got = z.run(c.wide)[0]
        assert np.array_equal(got, want), (c, "one call", _differs(got, want))
        z.reset()
        unit, at, parts = 64 * c.M, 0, []
        for u in c.cuts:
            parts.append(z.run(c.wide[at * unit:(at + u) * unit])[0])
            at += u
        got = np.concatenate(parts)
        assert np.array_equal(got, want), (c, "call cuts", _differs(got, want))
        z.close()


@pytest.mark.parametrize("place", [0, 7, 8])
def test_tile_slot_and_wave_do_not_matter(capi, P, corpus, eng, place):
    """The case's channel in slot 0, in slot 7, and ninth among eight fillers (slot 0 of a second tile, another wave):
    its bytes are the model's all the same, and so are the fillers'."""
    rng = np.random.default_rng(40 + place)
    for c in (c for c in corpus if c.family in ("low_order", "sat16", "tap_edges", "a_tie_1tap")):
        inc = rng.integers(0, 2 ** 32, 9).astype(np.uint64)
        shift = rng.integers(0, 9, 9).astype(np.uint8)
        inc[place], shift[place] = c.inc, c.L
        z = capi.Channelizer(eng, c.M, 9, taps=c.h)
        z.set_channels(0, phase_inc=inc, gain_shift=shift)
        got = z.run(c.wide)
        z.close()
        for ch in [place] + [k for k in range(9) if k != place]:
            want = cm.channel(c.wide, c.h, c.M, int(inc[ch]), int(shift[ch]), P)
            assert np.array_equal(got[ch], want), (c, "channel %d of 9, the case's is %d" % (ch, place), _differs(got[ch], want))


def test_taps_one_unit_over_the_bound_are_refused(capi, corpus, eng):
    """256 sum |h| = 2^31 - 256 runs (the sat16 cases above); the same taps with one unit more are IQD_EINVAL."""
    for kind in ("0deg", "45deg"):
        assert any(np.array_equal(c.h, cc.bound_taps(kind)) for c in corpus if c.family == "sat16")
        with pytest.raises(capi.IqdError) as err:
            capi.Channelizer(eng, 8, 1, taps=cc.over_bound_taps(kind))
        assert err.value.status == -1, err.value
    z = capi.Channelizer(eng, 8, 1, taps=cc.bound_taps("0deg"))   # nothing was left behind by the refusals
    assert np.array_equal(z.run(np.full(512, 128, np.uint8)), np.full((1, 64), 128, np.uint8))
    z.close()
