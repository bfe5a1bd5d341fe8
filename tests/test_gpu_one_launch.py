"""GPU (MI355X): small calls that the planner runs as ONE launch (iqd_stream_mixed.hip: mixed_stream_kernel - the AM, FM, SSB
and WBFM streaming pipelines as workgroup ranges of one grid), every channel of every call against the oracle.

The kernel is three variants (squelch magnitudes in the kernel, none, squelch-gated) times three WBFM rotation
instantiations; the at-size tests (tests/test_gpu_scale.py, 1410 to 16384 channels, a sample of channels, WBFM selector +1)
reach three of the nine bodies.  The planner needs no such size: 100 channels x 2^14 samples are one launch of 14
workgroups of three rings with 768-sample segments, which is what these cases run - all nine bodies, family subsets, the
smallest WBFM family and the smallest call, row lengths with short last segments and a ring filled exactly, warm segments
beside cold ones, the hand-overs between the one launch and the other arrangements, loud and quiet channels in one audio
wave.  With 20 WBFM channels of 22 segments the family's third workgroup holds 56 segments in its first ring and none in the
other two, so every case has rings that hold ids that are no segment.

Every case holds its shape to the host planning binding first (tests/one_launch_shapes.py; tests/test_host_planning.py pins
the same list without a GPU), runs through the C ABI with no path-pinning variable set, and asserts per call that
stats.mixed_launches rose by one and stats.stream_launches by the number of families.

Not reached here: the 16-byte PCM stores of the audio wave inside the one launch, which need WBFM segments of whole 512-sample
groups - the planner gives a one-launch call those from about a thousand channels up.  `bench.py --config 3` (819 / 819 / 819 /
1639 channels x 2^16) runs 3072-sample WBFM segments on rows of 2^16 samples and so takes them; at size they are covered by
tests/test_gpu_scale.py: test_config4_mixed_4096_channels_on_cu_shares (the same 3072-sample segments, a sample of channels
against the oracle), test_mixed_call_of_one_block_per_channel (3584) and test_mixed_1400_channels_at_the_share_threshold (1024)."""
import numpy as np
import pytest

import one_launch_shapes as S
from rtlsdrdiags_amd import synth

pytestmark = pytest.mark.gpu

PINS = ("IQD_MIXED", "IQD_RINGS", "IQD_STREAM_WGS", "IQD_WBFM_PATH", "IQD_D4_LEADFREE", "IQD_STREAM_MIN_SEG")
N_BASE = 7                                   # base rows: coprime to the 5 modes of the channel pattern and to the 64 lanes
LOUD_GAIN = 40 * 256000 / (2 * np.pi)        # tests/test_gpu_audio_wave.py: saturates the audio path, keeps the casts bounded
UNBOUNDED_GAIN = 6.0e9                       # tests/test_emu_wbfm.py: K so large that (int16)y can hit the indefinite value
assert np.float32(np.float32(UNBOUNDED_GAIN) / np.float32(75000.0)) * np.float32(32767.0) * 3.1730 >= 2.0 ** 31
# (the gains of tests/golden/cast_overflow.npz - 8e6 for WBFM - stay below the engine's bound: K 3.173 = 1.1e7)


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(autouse=True)
def no_pins(monkeypatch):
    for name in PINS:                        # (read when an engine is created)
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module")
def bases():
    """base(n) -> N_BASE seeded FM tones of n samples with different deviations and amplitudes plus one at deviation 75e3
    (the loud WBFM channels' row), made once per length for the whole file."""
    cache = {}

    def base(n):
        if n not in cache:
            rows = [synth.fm_tone(n, seed=2400 + k, deviation=2500.0 + 6100.0 * k, amplitude=30.0 + 6 * k) for k in range(N_BASE)]
            rows.append(synth.fm_tone(n, seed=2400 + N_BASE, deviation=75e3))
            cache[n] = rows
        return cache[n]
    return base


def plan(s, **kw):
    from test_host_planning import plan_call
    return S.hold(plan_call, s, **kw)


def layout(counts, wbfm_rot=1):
    """Channels in the pattern AM, FM, WBFM, LSB, USB while a family has channels left; the k-th channel of the AM / FM /
    SSB family has selector (+1, 0, -1)[k % 3], SSB is LSB and USB alternating.  wbfm_rot: one selector or one per channel
    of the family.  Returns (mode, selector, index in its family) per channel."""
    left, k, out = dict(counts), dict.fromkeys(S.FAMS, 0), []
    while any(left.values()):
        for f in ("am", "fm", "wbfm", "ssb", "ssb"):
            if not left[f]:
                continue
            i = k[f]
            if f == "wbfm":
                rot = wbfm_rot if isinstance(wbfm_rot, int) else wbfm_rot[i]
            else:
                rot = S.SELECTORS[i % 3]
            out.append((f if f != "ssb" else ("lsb", "usb")[i % 2], rot, i))
            left[f] -= 1
            k[f] += 1
    return out


def make_rows(base, n_ch, seed, loud=()):
    """Each channel one of the base rows rolled by its own offset, with a few bytes of its own in every 16 Ki samples."""
    rng = np.random.default_rng(seed)
    u8 = np.empty((n_ch, len(base[0])), np.uint8)
    for c in range(n_ch):
        u8[c] = np.roll(base[N_BASE if c in loud else c % N_BASE], 2 * ((c * 37) % 1009))
    for at in range(4000, u8.shape[1] - 16, 32768):
        u8[:, at:at + 16] = rng.integers(0, 256, size=(n_ch, 16), dtype=np.uint8)
    return u8


def plant_quiet_stretches(u8, seed, per_call_bytes, block_bytes=256, stretches=4):
    """2 to 5 blocks of digital silence at seeded places of every row, in every call"""
    rng = np.random.default_rng(seed)
    nblk = per_call_bytes // block_bytes
    for c in range(u8.shape[0]):
        for call in range(u8.shape[1] // per_call_bytes):
            for b0 in rng.integers(0, nblk - 6, stretches):
                at = call * per_call_bytes + block_bytes * int(b0)
                u8[c, at:at + block_bytes * int(rng.integers(2, 6))] = 128


class Rig:
    """An engine and one oracle chain per channel, fed the same calls."""

    def __init__(self, capi, oracle, chans, block_bytes=0, flags=0, threshold=None, gains=None):
        self.chans, self.n_ch, self.flags = chans, len(chans), flags
        self.block_bytes = block_bytes or 32768
        self.n_fams = len({m if m in ("am", "fm", "wbfm") else "ssb" for m, _, _ in chans})
        self.eng = capi.Engine(self.n_ch, block_bytes=block_bytes, flags=flags)
        self.chains = []
        for c, (mode, rot, _) in enumerate(chans):
            self.eng.set_mode(mode, first=c, n=1)
            self.eng.set_rotation(rot, first=c, n=1)
            o = oracle.chain()
            o.set_mode(mode)
            o.set_rotation(rot)
            self.chains.append(o)
        if threshold is not None:
            self.eng.set_squelch(threshold)
            for o in self.chains:
                o.set_squelch(threshold)
        for c, g in (gains or {}).items():
            self.set_wbfm_gain(c, g)
        self.dev = {}

    def set_wbfm_gain(self, c, g):
        self.eng.set_gain("wbfm", g, first=c, n=1)
        self.chains[c].set_gain(3, g)

    def set_rotation(self, c, rot):
        self.eng.set_rotation(rot, first=c, n=1)
        self.chains[c].set_rotation(rot)
        self.chans[c] = (self.chans[c][0], rot, self.chans[c][2])

    def _run_on_device_without_magnitudes(self, data):
        """iqd_accept_iq_device with a null magnitude pointer (tests/test_gpu_scale.py): with IQD_F_NO_MAGNITUDE the launch's
        variant that takes no squelch magnitudes."""
        eng, n_pcm = self.eng, data.shape[1] // 64
        if not self.dev:
            self.dev = {"iq": eng.dev_alloc(data.nbytes), "pcm": eng.dev_alloc(self.n_ch * n_pcm * 2), "cnt": eng.dev_alloc(self.n_ch * 4)}
        eng.dev_upload(self.dev["iq"], data)
        eng.dev_upload(self.dev["pcm"], np.zeros(self.n_ch * n_pcm, np.int16))
        eng.accept_device(self.dev["iq"], data.shape[1], self.dev["pcm"], self.dev["cnt"], 0)
        eng.synchronize()
        return (eng.dev_download(self.dev["pcm"], self.n_ch * n_pcm * 2, np.int16).reshape(self.n_ch, n_pcm),
                eng.dev_download(self.dev["cnt"], self.n_ch * 4, np.uint32), None, None)

    def call(self, tag, data, mixed=1, streams=None, on_device=False):
        """One call on the engine and on every chain; the counters' deltas (mixed None: left to the caller, in last_delta); every
        channel compared.  Returns the oracle's `allowed` flags [n_ch, blocks]."""
        data = np.ascontiguousarray(data)
        before = self.eng.stats()
        pcm, cnt, mag, allowed = self._run_on_device_without_magnitudes(data) if on_device else self.eng.accept(data)
        after = self.eng.stats()
        self.last_delta = (after["mixed_launches"] - before["mixed_launches"], after["stream_launches"] - before["stream_launches"])
        if mixed is not None:
            assert self.last_delta == (mixed, self.n_fams if streams is None else streams), \
                "%s: (mixed_launches, stream_launches) rose by %r" % (tag, self.last_delta)
        ref_allowed = []
        for c, (mode, rot, _) in enumerate(self.chans):
            ref, ref_mag, ref_al = self.chains[c].accept_stream(data[c], min(self.block_bytes, data.shape[1]))
            ref_allowed.append(ref_al)
            where = "%s, channel %d (%s, selector %+d)" % (tag, c, mode, rot)
            if allowed is not None:
                bad = np.flatnonzero(allowed[c] != ref_al)
                assert bad.size == 0, "%s: squelch decisions differ in blocks %s (%d in all)" % (where, bad[:8], bad.size)
            assert cnt[c] == len(ref), "%s: %d PCM samples, the oracle has %d" % (where, cnt[c], len(ref))
            bad = np.flatnonzero(pcm[c, :cnt[c]] != ref)
            assert bad.size == 0, "%s: PCM differs at %s (%d samples in all)" % (where, bad[:8], bad.size)
            if mag is not None:
                bad = np.flatnonzero(mag[c] != ref_mag)
                assert bad.size == 0, "%s: magnitudes differ in blocks %s (%d in all)" % (where, bad[:8], bad.size)
        return np.stack(ref_allowed)

    def close(self):
        st = self.eng.stats()
        for p in self.dev.values():
            self.eng.dev_free(p)
        self.eng.close()
        assert st["state_repairs"] == 0, st


def split_calls(u8, per_call_bytes):
    return [u8[:, at:at + per_call_bytes] for at in range(0, u8.shape[1], per_call_bytes)]


# ---- 1. the nine instantiations -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wbfm_rot", [1, 0, -1])
@pytest.mark.parametrize("variant", ["magnitudes", "no_magnitudes", "gated"])
def test_nine_instantiations(capi, oracle, bases, variant, wbfm_rot):
    """wbfm_stream_body<ROT, MAG, false, GATED> for ROT +1 / 0 / -1 in the launch's three variants: the 100-channel mix, two
    calls of 2^14 samples on one engine (the second starts from carried state).  gated: 128-sample blocks, quiet stretches of
    2 to 5 blocks that a threshold of -38 closes - channels of different lengths, segments cut on each channel's open blocks."""
    s = S.SHAPES["mix"]
    gated, flags = variant == "gated", 1 if variant == "no_magnitudes" else 0
    plan(s, wbfm_rot=wbfm_rot, gated=gated, flags=flags)
    n, chans = s.n, layout(s.counts, wbfm_rot)
    u8 = make_rows(bases(2 * n), len(chans), seed=10 + wbfm_rot)
    if gated:
        plant_quiet_stretches(u8, 20 + wbfm_rot, 2 * n)
    rig = Rig(capi, oracle, chans, block_bytes=256 if gated else 0, flags=flags, threshold=-38 if gated else None)
    closed = 0
    for k, data in enumerate(split_calls(u8, 2 * n)):
        ref_allowed = rig.call("%s, WBFM selector %+d, call %d" % (variant, wbfm_rot, k), data, on_device=variant == "no_magnitudes")
        if gated:
            assert (ref_allowed != 0).any(axis=1).all(), "call %d: a channel lost every block" % k
            closed += int(np.count_nonzero(ref_allowed == 0))
        else:
            assert ref_allowed.all()
    rig.close()
    if gated:
        assert closed > len(chans), closed       # the calls were gated in earnest


# ---- 2. family subsets ---------------------------------------------------------------------------------------------------
def _subset_cases():
    cases, at = [], 0
    for name in S.SUBSETS:
        if S.SHAPES[name].counts["wbfm"]:
            cases.append((name, S.SELECTORS[at % 3]))
            at += 1
        else:
            cases.append((name, 1))
    # seven subsets hold WBFM channels: two of them once more, so that each selector occurs three times
    return cases + [("subset_am_wbfm", 0), ("subset_wbfm_ssb", -1)]


SUBSET_CASES = _subset_cases()
assert all(sum(1 for n_, r in SUBSET_CASES if S.SHAPES[n_].counts["wbfm"] and r == sel) >= 3 for sel in S.SELECTORS)
assert {n_ for n_, _ in SUBSET_CASES} == set(S.SUBSETS) and len(S.SUBSETS) == 11


@pytest.mark.parametrize("name,wbfm_rot", SUBSET_CASES)
def test_family_subsets(capi, oracle, bases, name, wbfm_rot):
    """Every subset of two or more families, 40 channels each, as one launch: every order of the workgroup ranges, the
    launch without a WBFM range (whose sixteenth waves all leave at once) and without one of the other ranges."""
    s = S.SHAPES[name]
    plan(s, wbfm_rot=wbfm_rot)
    chans = layout(s.counts, wbfm_rot)
    u8 = make_rows(bases(2 * s.n), len(chans), seed=30 + len(name))
    rig = Rig(capi, oracle, chans)
    for k, data in enumerate(split_calls(u8, 2 * s.n)):
        rig.call("%s, WBFM selector %+d, call %d" % (name, wbfm_rot, k), data)
    rig.close()


# ---- 3. no smallest WBFM family exists; the smallest call does ---------------------------------------------------------
@pytest.mark.parametrize("name", ["wbfm_1", "wbfm_0", "mix_x18", "mix_x17"])
def test_no_wbfm_family_is_too_small_for_the_one_launch_but_a_call_is(capi, oracle, bases, name):
    """There is NO WBFM channel count w below which a call beside 60 AM, 60 FM and 120 SSB channels leaves the one launch, so
    this file has no "w - 1 must not fuse" run: the planner's size rule weighs the call, not the family
    (tests/test_host_planning.py holds every w from 1 to 60 to it).  ONE WBFM channel is still a range of the launch - its
    last workgroup: one ring of 22 segments, two without any (wbfm_1) - and without the channel the call is one launch of
    three families (wbfm_0).  The boundary that exists is the call's size: 18 + 18 + 18 + 36 channels are one launch
    (mix_x18), 17 + 17 + 17 + 34 run their tile kernels and equal the oracle all the same (mix_x17)."""
    s = S.SHAPES[name]
    _, streams = plan(s, wbfm_rot=0)
    assert (S.SMALLEST_WBFM, S.SMALLEST_MIX) == (1, 18)
    chans = layout(s.counts, 0)
    u8 = make_rows(bases(2 * s.n), len(chans), seed=40)
    rig = Rig(capi, oracle, chans)
    for k, data in enumerate(split_calls(u8, 2 * s.n)):
        rig.call("%s, call %d" % (name, k), data, mixed=1 if s.fused else 0, streams=None if s.fused else streams)
    rig.close()


# ---- 4. row lengths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,block_bytes", [("mix_16512", 256), ("mix_17024", 256), ("mix_49152", 0)])
def test_row_lengths(capi, oracle, bases, name, block_bytes):
    """16512 samples: the last segment has 384 samples; 17024: 128, shorter than the lead-in (both in 128-sample blocks);
    49152: exactly 64 segments per channel, so a channel fills a ring and no segment is short."""
    s = S.SHAPES[name]
    plan(s, wbfm_rot=-1)
    assert s.n - (s.segs - 1) * 768 == {"mix_16512": 384, "mix_17024": 128, "mix_49152": 768}[name]
    chans = layout(s.counts, -1)
    u8 = make_rows(bases(s.n), len(chans), seed=50)
    rig = Rig(capi, oracle, chans, block_bytes=block_bytes)
    rig.call(name, u8)
    rig.close()


def test_calls_of_three_one_and_two_blocks(capi, oracle, bases):
    """One engine, calls of 3, 1 and 2 blocks of 32768 bytes: from the second call on every channel's first segment is warm
    (it runs its lead-in through the decimators over carried samples) beside cold ones, in rings of their own and shared."""
    blocks = (3, 1, 2)
    names = {3: "mix_49152", 1: "mix", 2: "mix_32768"}
    for b in blocks:
        assert S.SHAPES[names[b]].n == b * 16384
        plan(S.SHAPES[names[b]], wbfm_rot=0)
    chans = layout(S.MIX, 0)
    u8 = make_rows(bases(sum(blocks) * 16384), len(chans), seed=60)
    rig = Rig(capi, oracle, chans)
    at = 0
    for k, b in enumerate(blocks):
        rig.call("call %d (%d blocks)" % (k, b), u8[:, at:at + b * 32768])
        at += b * 32768
    rig.close()


# ---- 5. arrangements taking over from each other -------------------------------------------------------------------------
def test_arrangements_take_over_from_each_other(capi, oracle, bases):
    """One engine, the 100-channel mix, the one launch and what replaces it in turn - a call this small that is not one launch
    runs every family's tile kernel - with every channel against the oracle at every step and the counters the plan predicts:
    WBFM channels of two selectors; a call that is not whole 128-sample units (one short block of 2^14 - 64 samples: a call of
    2^14 + 64 samples is 32896 bytes, 128.5 times 256: no multiple of any block size an engine can have (multiples of 256
    bytes), and longer than a short block may be, so iqd_accept_iq refuses it); a WBFM gain beyond the bound of the (int16) casts.  Once
    that gain is set back and the change has left the lead-ins' reach (one call of 2^14 samples: TAIL is 2048) the one launch
    must return - it did not before this test: the engine kept the largest gain a channel ever had."""
    n, rot0 = 1 << 14, 1
    chans = layout(S.MIX, rot0)
    rig = Rig(capi, oracle, chans)
    wbfm = [c for c, (m, _, _) in enumerate(chans) if m == "wbfm"]
    u8 = make_rows(bases(10 * n), len(chans), seed=70)
    at = [0]

    def step(tag, shape, samples=n):
        s = S.SHAPES[shape]
        assert s.n == samples
        _, streams = plan(s, wbfm_rot=rot0)
        data = u8[:, at[0]:at[0] + 2 * samples]
        at[0] += 2 * samples
        before = rig.eng.stats()["mixed_launches"]
        rig.call(tag, data, mixed=1 if s.fused else 0, streams=None if s.fused else streams)
        return rig.eng.stats()["mixed_launches"] - before

    step("(a) one launch", "mix")
    for c in wbfm[1::2]:
        rig.set_rotation(c, 0)
    step("(b) WBFM channels of two selectors", "mix_two_selectors")
    for c in wbfm[1::2]:
        rig.set_rotation(c, rot0)
    step("(c) one selector again", "mix")
    with pytest.raises(capi.IqdError, match="must be a positive multiple of block_bytes") as refused:
        rig.eng.accept(np.ascontiguousarray(u8[:, :2 * (n + 64)]))
    assert refused.value.status == -1        # IQD_EINVAL, before anything of the call was queued
    step("(d) one short block", "mix_short_block", samples=n - 64)
    step("(e) whole blocks again", "mix")
    usual = rig.eng.channel_gain(wbfm[7], "wbfm")
    rig.set_wbfm_gain(wbfm[7], UNBOUNDED_GAIN)
    step("(f) a WBFM gain beyond the cast bound", "mix_unbounded_gain")
    rig.set_wbfm_gain(wbfm[7], usual)
    step("(g) the gain set back: the change is in reach of the lead-ins", "mix_gain_change_in_reach")
    plan(S.SHAPES["mix"], wbfm_rot=rot0)
    back = False
    for k in range(2):                       # (3 calls at the most, the one above included: a condition, not a measurement)
        data = u8[:, at[0]:at[0] + 2 * n]
        at[0] += 2 * n
        rig.call("(g) call %d after the gain was set back" % (k + 2), data, mixed=None)
        if rig.last_delta[0]:
            assert rig.last_delta == (1, 4), rig.last_delta
            back = True
            break
        assert rig.last_delta == (0, 0), rig.last_delta
    assert back, "the one launch did not return within 3 calls of the gain being set back"
    step("(h) and stays", "mix")
    rig.close()


# ---- 6. loud and quiet WBFM channels in one audio wave -------------------------------------------------------------------
def test_loud_and_quiet_wbfm_channels_in_one_audio_wave(capi, oracle, bases):
    """Every third WBFM channel at a gain that saturates the audio path (|y2| > 16061: the decimator's clamp-after-every-MAC
    order) on a row of 75 kHz deviation, the others quiet: a ring of 64 segments holds almost three channels, so clamped and
    clamp-free segments share every ring of the audio wave and the rings' votes differ.  The gain keeps the casts bounded, so
    the calls are one launch: two of them, the loud end of the first in reach of the second's 40-tap window.  In front of them
    one call whose arrangement is left open: the engine of today counts gains set before the first call as a change in reach of
    the lead-ins and runs that call's tile kernels (a limitation of upload_params, no contract); its PCM is compared too."""
    s = S.SHAPES["mix"]
    plan(s, wbfm_rot=-1)
    chans = layout(s.counts, -1)
    loud = [c for c, (m, _, i) in enumerate(chans) if m == "wbfm" and i % 3 == 0]
    assert len(loud) == 7
    u8 = make_rows(bases(3 * s.n), len(chans), seed=80, loud=set(loud))
    rig = Rig(capi, oracle, chans, gains={c: LOUD_GAIN for c in loud})
    for k, data in enumerate(split_calls(u8, 2 * s.n)):
        if k == 0:
            rig.call("loud and quiet, the call after the gains were set", data, mixed=None)
        else:
            rig.call("loud and quiet, one launch, call %d" % k, data)
    rig.close()
