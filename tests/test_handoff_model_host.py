"""CPU tier: the hand-off predictor (tests/handoff_model.py) against the oracle, and every case of tests/repair_cases.py qualified
by it - the predicted set of bad hand-offs per call and channel, and that this set is what the case is for.  The boundaries
come from the planner (plan_call through the host planning binding, 256 CUs), so a planner change that would make a device
case vacuous fails here first.  tests/test_gpu_repairs.py runs the same rows."""
import numpy as np
import pytest

from rtlsdrdiags_amd import synth
from tests import emu_bind, handoff_model as H, repair_cases as R
from tests.test_host_planning import plan_call


@pytest.fixture(scope="module")
def L():
    return emu_bind.lib()


def test_the_deemphasis_model_is_the_oracles_recurrence(L, oracle):
    m = H.Deemph(L, oracle, synth.fm_tone(1 << 13, seed=5))
    y, up = H.iir_run(m.u, m.a1, np.float32(0), np.float32(0), 0, 2000)
    assert y.tobytes() == m.y[1999].tobytes() and up.tobytes() == m.u[1999].tobytes()
    # the vector form, from the stream's own zero start, lands on the exact states
    got = H.iir_cold(m.u, m.a1, [0, 0, 0], [1, 777, 2000])
    assert got.tobytes() == m.y[[0, 776, 1999]].tobytes()


@pytest.mark.parametrize("mode", ["am", "lsb", "usb"])
def test_the_detector_stream_getter_feeds_the_oracles_own_pcm(L, oracle, mode):
    """iqo_dc_stages is new with this model: its detector stream through the plain recurrence, gain and cast must be the
    chain's PCM, and its recurrence output the model's."""
    u8 = synth.am_tone(3 * 16384, seed=9, depth=0.8) if mode == "am" else synth.ssb_tone(3 * 16384, seed=9)
    st = oracle.dc_stages(H.rotated(oracle, u8, 1), mode)
    assert np.array_equal(st["det"], np.rint(st["det"])) and np.abs(st["det"]).max() > 10      # integers, and a live signal
    y = H.dc_serial(st["det"], H.consts(L)["dc_a1"])
    assert y.tobytes() == st["dc"].tobytes()
    o = oracle.chain()
    o.set_mode(mode)
    ref, _, _ = o.accept_stream(u8)
    pcm = np.array([oracle.cast_i16(np.float32(300.0) * v) for v in y], np.int16)
    assert np.array_equal(pcm, ref)


def test_the_tiny_state_rule():
    tiny, tiny2 = np.float32(2.0 ** -120), np.float32(-3e-45)
    assert H.agree(tiny, tiny2) and not H.agree(tiny, tiny2, tiny_ok=False) and H.agree(tiny, tiny, tiny_ok=False)
    assert not H.agree(np.float32(2.0 ** -100), tiny) and H.agree(np.float32(0.0), tiny2)
    assert not H.agree(np.float32(0.0), np.float32(-0.0), tiny_ok=False)                       # bit equality, as on the device
    assert H.agree_v([tiny, tiny, 1.0], [tiny2, tiny, 1.0], True).tolist() == [True, True, True]
    assert H.agree_v([tiny, tiny, 1.0], [tiny2, tiny, 1.0], False).tolist() == [False, True, True]


def test_the_starting_family_on_multiples_of_3072(L, oracle):
    """The table this model was first checked with: fm_tone(2^16, seed 5) with square stretches, boundaries at the multiples
    of 3072, lead-ins of 768 and 2048 samples ending at the boundary."""
    n = 1 << 16
    bounds = list(range(3072, n, 3072))
    rows = {"square": R.square(n), "then_fm": R.with_square(n, [(0, 20000)], 5),
            "stretches": R.with_square(n, [(5000, 7000), (30000, 34000)], 5), "late": R.with_square(n, [(20000, n)], 5)}
    want = {"square": (bounds, bounds), "then_fm": (bounds[:6], bounds[:6]), "stretches": ([6144, 33792], [33792]), "late": ([], [])}
    for name, u8 in rows.items():
        m = H.Deemph(L, oracle, u8)
        assert (m.bad_by_the_plain_rule(bounds, 768), m.bad_by_the_plain_rule(bounds, 2048)) == want[name], name


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_case_is_what_it_is_for(L, oracle, name):
    case = R.CASES[name]
    rows, pred = R.qualify(case, oracle, L, plan_call)
    assert len(rows) == case.n_calls == len(case.purpose)
    for k, p in enumerate(pred):
        for c, purpose in enumerate(case.purpose[k]):
            where = (name, "call", k, "channel", c, purpose, "bounds", p.bounds[c][:4], len(p.bounds[c]), "bad", p.bad[c], "flagged", p.flagged[c])
            assert R.purpose_holds(purpose, p.bounds[c], p.bad[c], p.flagged[c], k == 0), where
            assert set(p.flagged[c]) <= set(p.bounds[c])
            if case.modes[c] == "wbfm":
                # the first bad hand-off of a call is also the first one flagged: everything before it is exact
                assert (p.bad[c][:1] == p.flagged[c][:1]), where
                # the plain rule - ST_HALO / COLD_HALO zero-state steps ending AT the boundary - never calls a hand-off bad that the
                # device's own point of comparison accepts (a tile that has converged 768 samples before its start stays
                # converged), so `state_repairs` >= the predicted number holds under either reading
                assert set(p.plain[c]) <= set(p.bad[c]), (where, p.plain[c])
                if case.form != "tiles":
                    assert p.plain[c] == p.bad[c]
    if case.threshold is not None and case.kind == "wbfm":
        assert len(set(pred[0].vlen)) == len(pred[0].vlen), pred[0].vlen      # the open lengths differ from channel to channel


def test_periodic_envelopes_that_keep_two_dc_trajectories_apart(L, oracle):
    """The search behind the dc_*_periodic cases, at the default gain: noiseless square envelopes of period 2 .. 16 PCM samples,
    AM and USB, over a row of two DC tiles and a bit.  Most of them break a hand-off; the two chosen rows break both."""
    n = R.N_DC2
    broken = {}
    for mode, period, amp in R.PERIODIC_FAMILY:
        m = H.DcRemoval(L, oracle, R.periodic(n, mode, period, amp), mode)
        det = m.x[4096:4096 + 64 * period]
        assert np.array_equal(det[period:], det[:-period]), (mode, period)     # the detector stream has the period (or is constant)
        bad = m.bad(m.bounds(0, n // 32))
        if bad:
            broken[mode, period, amp] = len(bad)
    assert len(broken) == 19 and len(R.PERIODIC_FAMILY) == 30, sorted(broken)      # 19 of the 30 (recorded when the cases were made)
    assert all(broken.get(k) == 2 for k in R.PERIODIC_CHOSEN), broken
