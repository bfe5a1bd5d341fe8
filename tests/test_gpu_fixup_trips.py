"""GPU (MI355X): the WBFM boundary fix-up (iqd_stream_fix.h: wbfm_stream_fixup_body) - the launch behind the streaming kernel
that recomputes the first 21 PCM samples of every cold segment from the boundary records, as a kernel of its own and as a role
of the launch behind the one launch (iqd_kernels.hip: mixed_tail_kernel).

A workgroup takes 16 consecutive segments and stages their 17 records (the predecessor of the first included) with one
16-byte load per thread and a second one for 16 threads; the cases are the shapes at which that staging differs: the launch's
first workgroup (no predecessor record: staged one record further in), a full one, a short last one, a launch with no
boundary and with one, channel starts inside a workgroup and at its very start, a last segment with fewer than 21 PCM samples.
Quiet boundaries take the 40-tap sum without clamps, a loud row the reference's clamp after every MAC.

Every case pins the streaming path (IQD_F_WBFM_STREAM) and one workgroup of the streaming kernel (IQD_STREAM_WGS=1: read when
an engine is created, set the way tests/test_gpu_audio_wave.py sets it), holds the resulting shape to the host planning
binding, and compares PCM, counts and magnitudes with the oracle for equality."""
import numpy as np
import pytest

import one_launch_shapes as S
from rtlsdrdiags_amd import synth

pytestmark = pytest.mark.gpu

STREAM = 0x4                                 # IQD_F_WBFM_STREAM
LOUD_GAIN = 40 * 256000 / (2 * np.pi)        # tests/test_gpu_stream.py: test_loud_but_bounded_gain
PINS = ("IQD_MIXED", "IQD_RINGS", "IQD_STREAM_WGS", "IQD_WBFM_PATH", "IQD_D4_LEADFREE", "IQD_STREAM_MIN_SEG")
FIX_SEGS, FIX_PCM = 16, 21                   # iqd_stream_fix.h, iqd_stream.h: segments per fix-up workgroup, PCM samples per boundary


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(autouse=True)
def one_workgroup(monkeypatch):
    for name in PINS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("IQD_STREAM_WGS", "1")


def plan(n, channels, wgs=1):
    from test_host_planning import plan_call
    return plan_call(n, {"wbfm": (channels, True, False)}, flags=STREAM, stream_wgs=wgs)["fam"]["wbfm"]


def hold_shape(n, channels, segs):
    q = plan(n, channels)
    assert (q["path"], q["tile_len"], q["tiles_per_ch"], q["grid"], q["grouped"]) == (S.PLAN_STREAM, 768, segs, 1, 0), q
    return q


def wbfm_chain(oracle, gain=None):
    c = oracle.chain()
    c.set_mode("wbfm")
    if gain is not None:
        c.set_gain(3, gain)
    return c


def compare(tag, pcm, cnt, mag, c, ref, ref_mag):
    assert cnt[c] == len(ref), (tag, c, cnt[c], len(ref))
    bad = np.flatnonzero(pcm[c, :cnt[c]] != ref)
    assert bad.size == 0, (tag, c, bad[:8], bad.size)
    assert np.array_equal(mag[c], ref_mag), (tag, c)


@pytest.fixture(scope="module")
def tone_2p16(oracle):
    """One channel x 2^16 samples and the oracle's answers to its two halves as two calls, computed once (the first call's is
    also the answer to the single call of 2^15 samples)."""
    u8 = synth.fm_tone(1 << 16, seed=2601, deviation=48e3)
    chain = wbfm_chain(oracle)
    halves = [u8[:1 << 16], u8[1 << 16:]]
    return [(h,) + tuple(chain.accept_stream(h, 32768))[:2] for h in halves]


@pytest.mark.parametrize("calls", [1, 2])
def test_three_fixup_workgroups_and_a_ragged_last_segment(capi, tone_2p16, calls):
    """2^15 samples in one workgroup of the streaming kernel: 43 segments of 768 samples, so the fix-up's workgroups 0, 1 and 2
    stage 16 records one record in, 17, and 12; the last segment has 512 samples = 16 PCM samples, fewer than the 21 a
    boundary recomputes.  Two calls: the second one's first segment is warm and starts from the carried state."""
    n = 1 << 15
    hold_shape(n, 1, 43)
    assert [min(43 - w * FIX_SEGS, FIX_SEGS) + (1 if w else 0) for w in range(3)] == [16, 17, 12]
    assert (n - 42 * 768) // 32 == 16 < FIX_PCM
    eng = capi.Engine(1, flags=STREAM)
    eng.set_mode("wbfm")
    for k in range(calls):
        u8, ref, ref_mag = tone_2p16[k]
        pcm, cnt, mag, _ = eng.accept(u8)
        compare("call %d" % k, pcm, cnt, mag, 0, ref, ref_mag)
    st = eng.stats()
    eng.close()
    assert st["stream_launches"] == calls and st["state_repairs"] == 0, st


@pytest.mark.parametrize("n,segs", [(768, 1), (1536, 2)])
def test_no_boundary_and_exactly_one(capi, oracle, n, segs):
    hold_shape(n, 1, segs)
    u8 = synth.fm_tone(n, seed=2610 + segs, deviation=30e3)
    ref, ref_mag, _ = wbfm_chain(oracle).accept_stream(u8, 256)
    eng = capi.Engine(1, block_bytes=256, flags=STREAM)
    eng.set_mode("wbfm")
    pcm, cnt, mag, _ = eng.accept(u8)
    st = eng.stats()
    eng.close()
    compare(n, pcm, cnt, mag, 0, ref, ref_mag)
    assert st["stream_launches"] == 1 and st["state_repairs"] == 0 and st["state_checks"] == segs - 1, st


@pytest.mark.parametrize("n_ch", [5, 9])
def test_channel_starts_inside_and_at_the_start_of_a_fixup_workgroup(capi, oracle, n_ch):
    """Channels of 6 segments.  5 channels: 30 segments, the channels' first segments (ids 6, 12, 18, 24: not live, they have no
    predecessor) sit inside the two fix-up workgroups.  9 channels: 54 segments, and the fourth workgroup starts with id 48 =
    channel 8's first segment, so the predecessor record it stages belongs to channel 7 and must be left alone."""
    n = 4608
    hold_shape(n, n_ch, 6)
    starts = [6 * c for c in range(n_ch)]
    assert any(s % FIX_SEGS for s in starts[1:]) and (n_ch == 5 or any(s and s % FIX_SEGS == 0 for s in starts))
    rows = np.stack([synth.fm_tone(n, seed=2620 + c, deviation=9e3 + 7e3 * c, amplitude=30.0 + 9 * c) for c in range(n_ch)])
    eng = capi.Engine(n_ch, block_bytes=512, flags=STREAM)
    eng.set_mode("wbfm")
    pcm, cnt, mag, _ = eng.accept(rows)
    st = eng.stats()
    eng.close()
    for c in range(n_ch):
        ref, ref_mag, _ = wbfm_chain(oracle).accept_stream(rows[c], 512)
        compare(n_ch, pcm, cnt, mag, c, ref, ref_mag)
    assert st["stream_launches"] == 1 and st["state_repairs"] == 0 and st["state_checks"] == 5 * n_ch, st


def where_the_clamp_was_needed(oracle, u8, gain, ref):
    """The reference's last three stages from the oracle's own primitives (which must give the oracle's PCM), and beside them
    the 40-tap sum WITHOUT the clamp after every MAC: -> (PCM indices at which the two differ, the largest |y2|)."""
    s8 = (u8.astype(np.int16) - 128).astype(np.int8)
    w = oracle.wbfm_stages(oracle.rotate(s8, 1), gain=np.float32(gain))["w"]
    y2 = oracle.decimate_q15(oracle.taps_f32("wbfm_d2"), 4, oracle.decimate_q15(oracle.taps_f32("wbfm_d1"), 4, w))
    assert np.array_equal(oracle.decimate_q15(oracle.taps_f32("audio40"), 2, y2)[:len(ref)], ref)
    h = oracle.taps_q15("audio40").astype(np.int64)
    y2p = np.concatenate([np.zeros(39, np.int64), y2.astype(np.int64)])
    windows = np.lib.stride_tricks.sliding_window_view(y2p, 40)[1::2][:len(ref)]     # output k: y2[2k - 38 .. 2k + 1]
    free = ((1 << 14) + windows[:, ::-1] @ h) >> 15
    return np.flatnonzero(free != ref.astype(np.int64)), int(np.abs(y2.astype(np.int64)).max())


@pytest.mark.parametrize("tone,gain,n,segs,clamp_needed", [(20.0, LOUD_GAIN / 2, 1 << 15, 43, True), (1000.0, LOUD_GAIN, 6 * 16384, 128, False)])
def test_a_loud_row_takes_the_clamped_chain(capi, oracle, tone, gain, n, segs, clamp_needed):
    """A 20 Hz tone at 75 kHz deviation and half the gain of tests/test_gpu_stream.py: test_loud_but_bounded_gain: |y2| up to
    29 879, far above AUDIO40_SAFE = 16 061, for long stretches.  That the clamped chain was NEEDED behind a boundary is
    stated on the CPU: the 40-tap sum without the clamps, over the oracle's own stage-2 outputs, differs from the oracle's PCM
    in at least one of the 21 samples behind some boundary (PCM 389 and 589: segments 16 and 24).  The oracle's PCM alone
    cannot say it: the clamp acts on partial sums and no PCM sample of any row tried ends at the clamp's value.
    The second case is that test's own row and gain (1 kHz tone): its |y2| stays at 11 797, below AUDIO40_SAFE, so it is
    a quiet row whatever its name - kept as the case the clamp-free chain must get right at a large K."""
    hold_shape(n, 1, segs)
    u8 = synth.fm_tone(n, seed=5, deviation=75e3, tone=tone)
    ref, ref_mag, _ = wbfm_chain(oracle, gain).accept_stream(u8, 32768)
    differ, y2_max = where_the_clamp_was_needed(oracle, u8, gain, ref)
    behind = [int(k) for k in differ if k >= 24 and k % 24 < FIX_PCM]
    print("tone %g: max |y2| %d, the clamp changes %d PCM samples, behind a boundary: %s" % (tone, y2_max, differ.size, behind))
    assert (len(behind) >= 1 and y2_max > 16061) if clamp_needed else (differ.size == 0 and y2_max <= 16061)
    eng = capi.Engine(1, flags=STREAM)
    eng.set_mode("wbfm")
    eng.set_gain("wbfm", gain)
    pcm, cnt, mag, _ = eng.accept(u8)
    st = eng.stats()
    eng.close()
    compare("tone %g" % tone, pcm, cnt, mag, 0, ref, ref_mag)
    assert st["stream_launches"] == 1 and st["state_repairs"] == 0, st


def test_the_fixup_as_a_role_of_the_launch_behind_the_one_launch(capi, oracle, monkeypatch):
    """18 AM + 18 FM + 18 WBFM + 36 SSB channels x 2^14 samples, the smallest mix the planner runs as one launch (no pin): the
    WBFM family's 18 x 22 segments are 25 workgroups of mixed_tail_kernel that run the fix-up body; every third WBFM channel
    is loud.  Two calls; the first one's arrangement is left open (gains set before the first call count as a change in
    reach of the lead-ins: tests/test_gpu_one_launch.py), the second must be the one launch."""
    monkeypatch.delenv("IQD_STREAM_WGS")
    from test_host_planning import plan_call
    s = S.SHAPES["mix_x18"]
    S.hold(plan_call, s, wbfm_rot=1)
    chans = []
    for k in range(s.counts["ssb"]):
        chans += [(m, k) for m in ("am", "fm", "wbfm") if k < s.counts[m]] + [(("lsb", "usb")[k % 2], k)]
    n_ch = len(chans)
    assert n_ch == 90
    base = [synth.fm_tone(2 * s.n, seed=2640 + k, deviation=2500.0 + 6100.0 * k, amplitude=30.0 + 6 * k) for k in range(7)]
    base.append(synth.fm_tone(2 * s.n, seed=2647, deviation=75e3))
    loud = {c for c, (m, k) in enumerate(chans) if m == "wbfm" and k % 3 == 0}
    rows = np.stack([np.roll(base[7 if c in loud else c % 7], 2 * ((c * 37) % 1009)) for c in range(n_ch)])
    eng = capi.Engine(n_ch)
    chains = []
    for c, (mode, k) in enumerate(chans):
        rot = 1 if mode == "wbfm" else S.SELECTORS[k % 3]
        eng.set_mode(mode, first=c, n=1)
        eng.set_rotation(rot, first=c, n=1)
        o = oracle.chain()
        o.set_mode(mode)
        o.set_rotation(rot)
        if c in loud:
            eng.set_gain("wbfm", LOUD_GAIN, first=c, n=1)
            o.set_gain(3, LOUD_GAIN)
        chains.append(o)
    for call in range(2):
        part = np.ascontiguousarray(rows[:, 2 * s.n * call:2 * s.n * (call + 1)])
        before = eng.stats()["mixed_launches"]
        pcm, cnt, mag, _ = eng.accept(part)
        if call == 1:
            assert eng.stats()["mixed_launches"] - before == 1
        for c in range(n_ch):
            ref, ref_mag, _ = chains[c].accept_stream(part[c], 32768)
            compare("call %d, %s" % (call, chans[c][0]), pcm, cnt, mag, c, ref, ref_mag)
    st = eng.stats()
    eng.close()
    assert st["state_repairs"] == 0, st
