"""GPU (MI355X): the WBFM streaming kernel's audio wave (iqd_stream.hip: st_audio_wave) - the sixteenth wave of the workgroup,
which takes every piece's pair of stage-2 outputs from the IIR waves through a small LDS ring per IIR ring and runs the 40-tap
audio decimator, the PCM stores and the y2 parts of the boundary records for all three rings.

Every case pins the streaming path (IQD_F_WBFM_STREAM), compares PCM, counts and magnitudes with the oracle sample for sample
and asserts that no hand-off needed a repair (a wrong boundary record shows in the 21 PCM samples the fix-up recomputes, a
wrong pair, slot or position in the PCM behind it).  The planner gives small launches workgroups of ONE ring and 768-sample
segments; the cases that are about three rings side by side, or about segment lengths that allow the wide PCM stores, pin
the ring count and the number of workgroups the way the measurement runs do (IQD_RINGS, IQD_STREAM_WGS: read when an engine
is created) and hold the resulting plan to the host planning binding."""
import numpy as np
import pytest

from rtlsdrdiags_amd import synth

pytestmark = pytest.mark.gpu

STREAM = 0x4   # IQD_F_WBFM_STREAM
LOUD_GAIN = 40 * 256000 / (2 * np.pi)      # test_gpu_stream.py: test_loud_but_bounded_gain


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


def pin(monkeypatch, rings=None, wgs=None):
    for name, v in (("IQD_RINGS", rings), ("IQD_STREAM_WGS", wgs)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def plan(n, channels, rings=None, wgs=None, gated=False):
    from test_host_planning import plan_call
    return plan_call(n, {"wbfm": (channels, True, False)}, flags=STREAM, rings=rings or 0, stream_wgs=wgs or 0, gated=gated)["fam"]["wbfm"]


def oracle_chain(oracle, gain=None, rotation=1, threshold=None):
    c = oracle.chain()
    c.set_mode("wbfm")
    c.set_rotation(rotation)
    if gain is not None:
        c.set_gain(3, gain)
    if threshold is not None:
        c.set_squelch(threshold)
    return c


@pytest.fixture(scope="module")
def tone_2p20(oracle):
    """One channel x 2^20 samples (+ 640 for the row that is no multiple of 512: 128-sample squelch blocks there, a row is
    whole blocks) and the oracle's answers, computed once: {samples: (bytes, block_bytes, PCM, magnitudes)}."""
    u8 = synth.fm_tone((1 << 20) + 640, seed=1601, deviation=55e3)
    out = {}
    for n, block_bytes in ((1 << 20, 32768), ((1 << 20) + 640, 256)):
        out[n] = (u8[:2 * n], block_bytes) + tuple(oracle_chain(oracle).accept_stream(u8[:2 * n], block_bytes))[:2]
    return out


def run_one(capi, u8, block_bytes, ref, ref_mag):
    eng = capi.Engine(1, block_bytes=block_bytes, flags=STREAM)
    eng.set_mode("wbfm")
    pcm, cnt, mag, _ = eng.accept(u8)
    st = eng.stats()
    eng.close()
    assert st["stream_launches"] == 1 and st["state_repairs"] == 0, st
    assert cnt[0] == len(ref)
    bad = np.flatnonzero(pcm[0, :cnt[0]] != ref)
    assert bad.size == 0, (bad[:8], bad.size)
    assert np.array_equal(mag[0], ref_mag)


@pytest.mark.parametrize("rings", [None, 1, 2, 3])
def test_ring_depth_and_ring_counts_on_one_long_row(capi, monkeypatch, tone_2p20, rings):
    """1 366 segments of 768 samples, 48 pieces each - far more than a y2 ring holds - in workgroups of one, two and three
    rings (None: the planner's own choice, one); the audio wave must skip the rings that are not there.  768-sample segments
    take the 8-byte PCM stores; the last segment (256 samples) is shorter than the lead-in."""
    q = plan(1 << 20, 1, rings=rings)
    assert (q["rings"], q["tile_len"], q["rounds"]) == (rings or 1, 768, 1) and q["grid"] * q["rings"] * 64 >= 1366, q
    pin(monkeypatch, rings=rings)
    u8, block_bytes, ref, ref_mag = tone_2p20[1 << 20]
    run_one(capi, u8, block_bytes, ref, ref_mag)


def test_two_rings_by_the_planners_own_choice(capi, oracle, monkeypatch):
    """A launch of 2 x 10^7 samples runs workgroups of two rings by the planner's own choice.  (Its own three-ring launches
    start at twice that - more than a host call hands over in one launch: the 2^28-sample row of tests/test_gpu_scale.py and the
    bench paths run them.)"""
    n_ch, rings = 600, 2
    n = 1 << 15
    assert plan(n, n_ch)["rings"] == rings
    pin(monkeypatch)
    base = [synth.fm_tone(n, seed=1700 + k, deviation=8e3 + 9e3 * k, amplitude=30.0 + 11 * k) for k in range(7)]   # (7 and 64 lanes: coprime)
    refs = [oracle_chain(oracle).accept_stream(b, 32768) for b in base]
    eng = capi.Engine(n_ch, flags=STREAM)
    eng.set_mode("wbfm")
    pcm, cnt, mag, _ = eng.accept(np.stack([base[c % 7] for c in range(n_ch)]))
    st = eng.stats()
    eng.close()
    assert st["stream_launches"] == 1 and st["state_repairs"] == 0, st
    for c in range(n_ch):
        ref, ref_mag, _ = refs[c % 7]
        assert cnt[c] == len(ref) and np.array_equal(pcm[c, :cnt[c]], ref), c
        assert np.array_equal(mag[c], ref_mag), c


def test_loud_and_quiet_channels_in_neighbouring_rings(capi, oracle, monkeypatch):
    """96 channels x 2^15, every third at a gain that saturates the audio path (|y2| > 16061: the decimator's clamp-after-every-
    MAC order), in workgroups of three rings: a ring is 64 consecutive segments, about a channel and a half, so clamped and
    clamp-free rings sit side by side in one audio wave and each must keep its own vote.  Two calls: a loud stretch at the
    end of the first call is still in reach of the 40-tap window at the start of the second (the carried histories)."""
    n_ch, n = 96, 1 << 15                                # (gain and deviation of test_gpu_stream.py: test_loud_but_bounded_gain)
    assert plan(n, n_ch, rings=3)["rings"] == 3
    pin(monkeypatch, rings=3)
    rows = np.stack([synth.fm_tone(2 * n, seed=1800 + c % 5, deviation=75e3 if c % 3 == 0 else 20e3 + 500 * c) for c in range(n_ch)])
    eng = capi.Engine(n_ch, flags=STREAM)
    eng.set_mode("wbfm")
    chains = []
    for c in range(n_ch):
        if c % 3 == 0:
            eng.set_gain("wbfm", LOUD_GAIN, first=c, n=1)
        chains.append(oracle_chain(oracle, gain=LOUD_GAIN if c % 3 == 0 else None))
    for call in range(2):
        part = rows[:, 2 * n * call:2 * n * (call + 1)]
        pcm, cnt, mag, _ = eng.accept(part)
        for c in range(n_ch):
            ref, ref_mag, _ = chains[c].accept_stream(part[c], 32768)
            assert cnt[c] == len(ref) and np.array_equal(pcm[c, :cnt[c]], ref), (call, c, np.flatnonzero(pcm[c, :cnt[c]] != ref)[:8])
            assert np.array_equal(mag[c], ref_mag), (call, c)
    st = eng.stats()
    eng.close()
    assert st["stream_launches"] == 2 and st["state_repairs"] == 0, st


@pytest.mark.parametrize("rings", [None, 3])
def test_fast_and_slow_rings_side_by_side(capi, oracle, monkeypatch, rings):
    """Three calls of 5, 1 and 7 blocks on one engine: a warm first segment in every call (its ring runs the lead-in through
    the decimators and hands pairs over from the first piece), rings of cold full segments beside it (which hand over from
    position 0), a last segment shorter than the lead-in with the keeper of the restart state before it (5 blocks = 106
    segments + 512 samples).  A ring's six waves - four P waves, the IIR wave, the audio wave - must agree on its lead-in."""
    pin(monkeypatch, rings=rings)
    blocks = (5, 1, 7)
    u8 = synth.fm_tone(sum(blocks) * 16384, seed=1900, deviation=60e3)
    chain = oracle_chain(oracle)
    eng = capi.Engine(1, flags=STREAM)
    eng.set_mode("wbfm")
    off = 0
    for k, b in enumerate(blocks):
        part = u8[off:off + b * 32768]
        off += b * 32768
        ref, ref_mag, _ = chain.accept_stream(part, 32768)
        pcm, cnt, mag, _ = eng.accept(part)
        assert cnt[0] == len(ref) and np.array_equal(pcm[0, :cnt[0]], ref), (k, np.flatnonzero(pcm[0, :cnt[0]] != ref)[:8])
        assert np.array_equal(mag[0], ref_mag), k
    st = eng.stats()
    eng.close()
    assert st["stream_launches"] == 3 and st["state_repairs"] == 0, st


@pytest.mark.parametrize("wide", [False, True])
def test_rotation_groups_then_a_gated_call(capi, oracle, monkeypatch, wide):
    """48 channels x 2^15 with the rotation selectors +1 / 0 / -1 mixed: the grouped instantiation (segment ids padded per
    group, so some rings hold ids that are no segment).  Then the same engine with a squelch that closes some 128-sample
    blocks: the gated instantiation, channels of different lengths, last segments that end anywhere on the 128-sample grid.
    wide: four workgroups of three rings, 2048-sample segments - the 16-byte PCM stores, whose ragged ends the gated call
    reaches; else the planner's own 768-sample segments and 8-byte stores."""
    n_ch, n = 48, 1 << 15
    kw = dict(rings=3, wgs=4) if wide else {}
    q = plan(n, (16, 16, 16), **kw)
    assert q["grouped"] == 1 and q["tile_len"] == (2048 if wide else 768), q
    pin(monkeypatch, **kw)
    rng = np.random.default_rng(21)
    rots = [1, 0, -1] * 16
    rng.shuffle(rots)
    rows = np.stack([synth.fm_tone(n, seed=2000 + c % 6, deviation=30e3 + 700 * c, amplitude=30.0 + c, sigma=1.0) for c in range(n_ch)])
    gated_rows = rows.copy()
    for c in range(n_ch):                                # quiet stretches of a few blocks: the squelch drops all but the first of each
        for b0 in rng.integers(0, n // 128 - 6, 5):
            gated_rows[c, 256 * int(b0):256 * (int(b0) + int(rng.integers(2, 6)))] = 128
    eng = capi.Engine(n_ch, block_bytes=256, flags=STREAM)
    eng.set_mode("wbfm")
    chains = [oracle_chain(oracle, rotation=rots[c]) for c in range(n_ch)]
    for c in range(n_ch):
        eng.set_rotation(rots[c], first=c, n=1)
    closed = 0
    for call, data in enumerate((rows, gated_rows)):
        if call == 1:
            eng.set_squelch(-38)
            for ch in chains:
                ch.set_squelch(-38)
        pcm, cnt, mag, allowed = eng.accept(data)
        for c in range(n_ch):
            ref, ref_mag, ref_allowed = chains[c].accept_stream(data[c], 256)
            assert np.array_equal(allowed[c], ref_allowed), (call, c)
            assert cnt[c] == len(ref) and np.array_equal(pcm[c, :cnt[c]], ref), (call, c, rots[c], np.flatnonzero(pcm[c, :cnt[c]] != ref)[:8])
            assert np.array_equal(mag[c], ref_mag), (call, c)
            closed += int(np.count_nonzero(np.asarray(ref_allowed) == 0)) if call == 1 else 0
    st = eng.stats()
    eng.close()
    assert st["stream_launches"] == 2 and st["state_repairs"] == 0, st
    assert closed > n_ch        # the second call was gated


@pytest.mark.parametrize("n,is_wide", [(1 << 20, True), ((1 << 20) + 640, False)])
def test_both_pcm_store_shapes(capi, monkeypatch, tone_2p20, n, is_wide):
    """Four workgroups of three rings, 1536-sample segments (whole 512-sample groups).  2^20 samples: rows of whole 32-byte
    sectors - the audio wave collects 256 samples per 16-byte store; the last segment has 1024 samples.  2^20 + 640: the row
    length is no multiple of 512 samples, so no row but the first is aligned and the PCM leaves 8 bytes at a time; the last
    segment has 128 samples.  (768-sample segments, the other way to the 8-byte stores: the first test of this file.)"""
    q = plan(n, 1, rings=3, wgs=4)
    assert (q["rings"], q["tile_len"], q["grid"]) == (3, 1536, 4), q
    assert (q["tile_len"] % 512 == 0 and n % 512 == 0) == is_wide
    assert n - (q["tiles_per_ch"] - 1) * q["tile_len"] == (1024 if is_wide else 128)
    pin(monkeypatch, rings=3, wgs=4)
    u8, block_bytes, ref, ref_mag = tone_2p20[n]
    run_one(capi, u8, block_bytes, ref, ref_mag)
