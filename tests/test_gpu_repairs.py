"""GPU (MI355X): the exact-state repair paths, reached on purpose in every launch form and held to a CPU prediction.

Interior WBFM tiles and segments and the tiles of the many-wave DC pass warm up from the zero state; the device verifies every
hand-off bit for bit and re-runs what does not chain up (wbfm_repair_body<GATED> behind wbfm_verify_kernel or the streaming
fix-up's check; dc_tiled_kernel -> dc_chainup_kernel -> the flagged branch of dc_redo_kernel; the `again` loop of dc_block_wave).
A wrong repair is an ulp-sized state error on an unusual input, so every case here
  * runs rows built to break chosen hand-offs (tests/repair_cases.py), whose bad hand-offs tests/handoff_model.py predicts on
    the CPU from the planner's own boundaries (tests/test_handoff_model_host.py asserts, without a GPU, that every case is what
    it is for); the case holds its shape to the planner first and fails loudly if the planner has moved;
  * compares PCM, magnitudes, squelch flags and counts of every channel with the oracle, call by call;
  * reads the counters around every call: `state_repairs` rises by at least the predicted number of bad hand-offs (and at
    least 1) where there are any - by exactly that number on the tile kernel, which re-runs a bad tile and nothing else - and by
    exactly 0 on a call the model calls clean, also straight after a repaired one (the repair and redo flags are zero between
    calls); `state_checks` rises by the hand-offs minus those the first look flags; `stream_launches` / `mixed_launches` prove
    the form that ran.  DC removal: a flagged channel is redone as a whole, once, so the count there is flagged CHANNELS.

Launch forms (case names of tests/repair_cases.py):
  tile kernel, verify_at_end 0        wbfm_tiles, wbfm_tiles_gated (GATED), wbfm_in_a_row_tiles, wbfm_k_*_tiles
  streaming, verify_at_end 1          wbfm_stream (the redo_next rule), wbfm_short_last[_min_seg_1] (the keeper rule of a short
                                      last segment, wbfm_pick_carry), wbfm_in_a_row_stream, wbfm_k_*_stream
  streaming gated, verify_at_end 2    wbfm_stream_gated (hand-offs counted on the device)
  one launch (mixed kernel)           mixed_one_launch: repaired and clean WBFM channels beside AM / FM / SSB families
  DC removal, many waves              dc_{am,usb}[_gated]_{at,above}_1e6, dc_am_middle_of_three, dc_{am,usb}_periodic (CNT_DC_REDO)
  DC removal, one wave in place       dc_again_loop (no counter: PCM; tests/test_emu_chains.py shows the loop running on the host)

Mutation check (by hand, once, on a scratch copy, nothing of it committed; this file alone on each mutant; healthy tree: 30 passed):
  (a) wbfm_repair_body with `redo_next` always false (neither the segment behind a re-run one nor the short last segment behind a
      re-run keeper is run again): 5 RED, 25 green.
        test_wbfm_launch_form[wbfm_stream_loud], [wbfm_stream_gated_loud]   channel 1 (bad, then good), call 0: the first 7 PCM
                                                                            samples of the segment behind the last re-run one
        test_short_last_segment[0-True], [1-True]                           channel 0, the NEXT call's PCM samples 0..3
        test_one_launch_mixed_kernel                                        channel 22 (bad hand-off in front of the short last
                                                                            segment), the next call's PCM sample 0
      Green at the default gain (an ulp of state does not reach a sample there: hence the loud variants) and on the tile kernel,
      which has no such rule.
  (b) dc_redo_kernel always takes the unflagged branch: 9 RED (every test_dc_redo case with a flagged channel), 21 green.
        dc_{am,usb}_above_1e6, dc_{am,usb}_gated_above_1e6, dc_am_middle_of_three, dc_{am,usb}_periodic: a state_repairs delta of 0
        where 1 is predicted (their PCM is unchanged: gain x a denormal is 0, and at gain 300 an ulp of y does not reach the cast)
        dc_{am,usb}_periodic_loud: 8704 wrong PCM samples, from the first one of the second DC tile on"""
import numpy as np
import pytest

from tests import emu_bind, repair_cases as R

pytestmark = pytest.mark.gpu

PINS = ("IQD_MIXED", "IQD_RINGS", "IQD_STREAM_WGS", "IQD_WBFM_PATH", "IQD_D4_LEADFREE", "IQD_STREAM_MIN_SEG", "IQD_NO_DET16")
COUNTERS = ("state_repairs", "state_checks", "segment_repairs", "stream_launches", "mixed_launches")


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(autouse=True)
def no_pins(monkeypatch):
    for name in PINS:                        # (read when an engine is created)
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def prepared(oracle):
    """case name -> (rows per call, prediction per call): held to the planner, made once per case, shared, left unchanged"""
    from test_host_planning import plan_call
    L = emu_bind.lib()
    cache = {}

    def get(name):
        if name not in cache:
            rows, pred = R.qualify(R.CASES[name], oracle, L, plan_call)      # (asserts the launch form the case is for)
            for r in rows:
                r.setflags(write=False)
            cache[name] = (rows, pred)
        return cache[name]
    return get


class Rig:
    """An engine and one oracle chain per channel, fed the same calls; the counters' deltas per call."""

    def __init__(self, capi, oracle, case, rotations=None):
        self.case, self.n_ch = case, len(case.modes)
        self.block = case.block_bytes or 32768
        self.eng = capi.Engine(self.n_ch, block_bytes=case.block_bytes, flags=case.flags)
        self.chains = []
        for c, mode in enumerate(case.modes):
            rot = rotations[c] if rotations else 1
            self.eng.set_mode(mode, first=c, n=1)
            self.eng.set_rotation(rot, first=c, n=1)
            o = oracle.chain()
            o.set_mode(mode)
            o.set_rotation(rot)
            self.chains.append(o)
        if case.threshold is not None:
            self.eng.set_squelch(case.threshold)
            for o in self.chains:
                o.set_squelch(case.threshold)
        for c, (demod, gain) in case.gains.items():
            self.eng.set_gain(demod, float(gain), first=c, n=1)
            self.chains[c].set_gain({"am": 1, "fm": 2, "wbfm": 3, "ssb": 4}[demod], float(gain))
        self.eng.set_profiling(True)         # (the calls read the device counters back)

    def call(self, tag, data):
        """One call on the engine and on every chain, every channel compared; returns the counters' deltas."""
        data = np.ascontiguousarray(data)
        before = self.eng.stats()
        pcm, cnt, mag, allowed = self.eng.accept(data)
        after = self.eng.stats()
        delta = {k: int(after[k]) - int(before[k]) for k in COUNTERS}
        for c, mode in enumerate(self.case.modes):
            ref, ref_mag, ref_al = self.chains[c].accept_stream(data[c], min(self.block, data.shape[1]))
            where = "%s, channel %d (%s), counters %r" % (tag, c, mode, delta)
            bad = np.flatnonzero(allowed[c] != ref_al)
            assert bad.size == 0, "%s: squelch decisions differ in blocks %s (%d in all)" % (where, bad[:8], bad.size)
            assert cnt[c] == len(ref), "%s: %d PCM samples, the oracle has %d" % (where, cnt[c], len(ref))
            bad = np.flatnonzero(pcm[c, :cnt[c]] != ref)
            assert bad.size == 0, "%s: PCM differs at %s (%d samples in all)" % (where, bad[:8], bad.size)
            bad = np.flatnonzero(mag[c] != ref_mag)
            assert bad.size == 0, "%s: magnitudes differ in blocks %s (%d in all)" % (where, bad[:8], bad.size)
        return delta

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()


def expected(case, p):
    """(lower bound of the state_repairs delta, exact?, state_checks delta or None) of one call from its prediction"""
    if case.kind == "dc":
        return sum(1 for f in p.flagged if f), True, 0          # one redo per flagged channel; the DC pass counts no checks
    n_bad, n_flagged = sum(len(b) for b in p.bad), sum(len(f) for f in p.flagged)
    return n_bad, case.form == "tiles" or n_bad == 0, p.handoffs - n_flagged


def check_call(case, k, p, delta, launches):
    tag = "%s call %d" % (case.name, k)
    want, exact, checks = expected(case, p)
    print("REPAIRS %s: segments of %d, %d hand-offs, predicted bad %s, flagged %s -> %r"
          % (tag, p.tile_len, p.handoffs, [len(b) for b in p.bad if b] or 0, [len(f) for f in p.flagged if f] or 0, delta))
    assert (delta["stream_launches"], delta["mixed_launches"]) == launches, (tag, delta)
    if want == 0:
        assert delta["state_repairs"] == 0, (tag, "a clean call", delta)
    else:
        assert delta["state_repairs"] >= max(1, want), (tag, want, delta)
        if exact:
            assert delta["state_repairs"] == want, (tag, want, delta)
    if checks is not None:
        assert delta["state_checks"] == checks, (tag, checks, delta)
    return delta


def run_case(capi, oracle, prepared, name, launches, rotations=None):
    case = R.CASES[name]
    rows, pred = prepared(name)
    with Rig(capi, oracle, case, rotations) as rig:
        deltas = [check_call(case, k, pred[k], rig.call("%s call %d" % (name, k), rows[k]), launches) for k in range(len(rows))]
    assert any(d["state_repairs"] > 0 for d in deltas) == any(expected(case, p)[0] for p in pred)
    return deltas


# ---- WBFM forms 1 - 4: all bad / bad then good / isolated / none in one call, then a clean call ------------------------------------
@pytest.mark.parametrize("name", [n for n in R.CASES if n.startswith(("wbfm_tiles", "wbfm_stream"))])
def test_wbfm_launch_form(capi, oracle, prepared, name):
    """Four channels - every hand-off bad, bad ones then good ones, two isolated bad ones, none - then a clean call; at the
    default gain and at 5e8, where an ulp of state is a unit of the sample."""
    deltas = run_case(capi, oracle, prepared, name, (1, 0) if "stream" in name else (0, 0))
    # the re-runs go through the tile kernel's body, whose own segmented recurrence has to go round again on the square pattern
    assert deltas[0]["segment_repairs"] > 0, deltas[0]
    if "stream" in name:                     # (a clean streamed call runs no tile body at all)
        assert deltas[1]["segment_repairs"] == 0, deltas[1]


# ---- 6. a short last segment behind a bad hand-off: the keeper rule -----------------------------------------------------------------
@pytest.mark.parametrize("loud", [False, True])
@pytest.mark.parametrize("min_seg", [0, 1])
def test_short_last_segment(capi, oracle, prepared, monkeypatch, min_seg, loud):
    """The hand-off into segment ntiles - 2 is bad and the last segment is shorter than FORCED_BACK: the re-run rewrites the record
    that kept the channel's restart state, the last segment is re-run with it, and the next call (clean FM) continues exactly."""
    if min_seg:
        monkeypatch.setenv("IQD_STREAM_MIN_SEG", "1")
    name = "wbfm_short_last" + ("_min_seg_1" if min_seg else "") + ("_loud" if loud else "")
    rows, pred = prepared(name)
    assert pred[0].vlen[0] % pred[0].tile_len < 768 and pred[0].bad[0] == [pred[0].bounds[0][-2]]
    run_case(capi, oracle, prepared, name, (1, 0))


# ---- 7. repaired calls in a row, the same stream through a streaming and a tile-kernel engine ---------------------------------------
def test_repaired_calls_in_a_row_on_both_kernels(capi, oracle, prepared):
    """Three repaired calls and a clean one over one stream, every call given to a streaming engine and to a tile-kernel engine
    (the arrangement of tests/test_gpu_stream.py::test_alternating_with_the_tile_kernel): the restart state a repaired call
    carries out is exact, whichever kernel continues."""
    names = ("wbfm_in_a_row_stream", "wbfm_in_a_row_tiles")
    prep = [prepared(n) for n in names]
    assert all(np.array_equal(a, b) for a, b in zip(prep[0][0], prep[1][0]))
    with Rig(capi, oracle, R.CASES[names[0]]) as streamed, Rig(capi, oracle, R.CASES[names[1]]) as tiled:
        for k in range(len(prep[0][0])):
            for name, rig, (rows, pred) in zip(names, (streamed, tiled), prep):
                check_call(R.CASES[name], k, pred[k], rig.call("%s call %d" % (name, k), rows[k]), (1, 0) if rig.case.form == "stream" else (0, 0))


# ---- 8. K < 1: no sub-2^-100 exception ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["stream", "tiles"])
def test_k_below_one(capi, oracle, prepared, form):
    """A modulated stretch, then the noiseless carrier for the rest of the call and the whole next one.  At the default gain the
    second call's hand-offs agree by the exception (a delta of exactly 0); at gain 1.0, K < 1, every one of them is repaired."""
    launches = (1, 0) if form == "stream" else (0, 0)
    below = run_case(capi, oracle, prepared, "wbfm_k_below_1_" + form, launches)
    default = run_case(capi, oracle, prepared, "wbfm_k_default_" + form, launches)
    n = len(prepared("wbfm_k_below_1_" + form)[1][1].bounds[0])
    assert below[1]["state_repairs"] >= n and default[1]["state_repairs"] == 0


# ---- 5. the one-launch mixed kernel -------------------------------------------------------------------------------------------------
def test_one_launch_mixed_kernel(capi, oracle, prepared):
    import one_launch_shapes as S
    assert R.CASES["mixed_one_launch"].modes.count("wbfm") == S.SHAPES[R.MIXED_SHAPE].counts["wbfm"]
    deltas = run_case(capi, oracle, prepared, "mixed_one_launch", (4, 1), rotations=[rot for _, rot in R.mixed_layout()])
    assert deltas[0]["state_repairs"] > 0 and deltas[1]["state_repairs"] == 0


# ---- 9 / 10. DC removal: the chain-up check and the flagged branch of dc_redo_kernel (CNT_DC_REDO) ---------------------------------
DC_CASES = [n for n, c in R.CASES.items() if c.kind == "dc" and c.form == "dc"]


@pytest.mark.parametrize("name", DC_CASES)
def test_dc_redo(capi, oracle, prepared, name):
    """AM-only / SSB-only engines: `state_repairs` shows CNT_DC_REDO alone.  One redo per flagged channel, none for its
    neighbours, none on the clean call that follows (the per-channel redo flags are cleared)."""
    deltas = run_case(capi, oracle, prepared, name, (0, 0))
    flagged = sum(1 for f in prepared(name)[1][0].flagged if f)
    assert deltas[0]["state_repairs"] == flagged and deltas[1]["state_repairs"] == 0
    assert ("above" in name or "periodic" in name or "middle" in name) == (flagged > 0)


# ---- 11. the `again` loop of dc_block_wave, in place behind the streaming pipeline -------------------------------------------------
def test_dc_again_loop_in_place(capi, oracle, prepared):
    """One DC tile, streamed, the pass in place over int16 detector values, bit equality the rule (gain above 1e6): the wave's
    segments go round again in the constant part.  No counter shows it; the PCM must be the oracle's."""
    run_case(capi, oracle, prepared, "dc_again_loop", (1, 0))
