"""GPU (MI355X): the per-piece bookkeeping of the WBFM streaming kernel's P waves (iqd_stream.hip: st_p_wave) - the clamped
position of the next input request and its move from the kept tail to the call's samples, the ring-room test, the squelch
magnitudes' group sums, and the order (u0, u2, u1, u3) of a 16-byte ring chunk, which the IIR wave reads in its lead-in
(st_iir_lead_in: rings of cold full segments) and in its piece path (st_iir_piece: every other ring).

Every case pins the streaming path (IQD_F_WBFM_STREAM), compares PCM, counts and magnitudes with the oracle sample for sample
and asserts that no hand-off needed a repair.  Small shapes: the planner gives them 768-sample segments."""
import numpy as np
import pytest

from rtlsdrdiags_amd import synth
from test_gpu_audio_wave import STREAM, oracle_chain, pin, plan, run_one

pytestmark = pytest.mark.gpu

N_CH, N = 40, 1 << 13


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


def channel_rows(sigma=0.0):
    """40 channels x 2^13 samples, each with its own data."""
    return np.stack([synth.fm_tone(N, seed=2300 + c, deviation=12e3 + 1500 * c, amplitude=25.0 + 2 * c, sigma=sigma) for c in range(N_CH)])


@pytest.fixture(scope="module")
def plain_rows(oracle):
    """The 40 rows and the oracle's answers at rotation +1 with 256-byte blocks, computed once."""
    rows = channel_rows()
    return rows, [oracle_chain(oracle).accept_stream(rows[c], 256) for c in range(N_CH)]


def check_rows(eng, data, refs, launches=1):
    pcm, cnt, mag, allowed = eng.accept(data)
    st = eng.stats()
    assert st["stream_launches"] == launches and st["state_repairs"] == 0, st
    for c, (ref, ref_mag, ref_allowed) in enumerate(refs):
        assert np.array_equal(allowed[c], ref_allowed), c
        assert cnt[c] == len(ref), (c, cnt[c], len(ref))
        bad = np.flatnonzero(pcm[c, :cnt[c]] != ref)
        assert bad.size == 0, (c, bad[:8], bad.size)
        assert np.array_equal(mag[c], ref_mag), c


def test_clamp_ragged_end_and_the_waves_last_lanes(capi, oracle, monkeypatch):
    """One channel of 2^17 + 640 samples with 256-byte blocks: 172 segments, the last of 384 samples - shorter than the lead-in,
    so its lanes' requests stop advancing in the middle of the run while the 15 other segments of its P wave go on, and the
    groups behind its end must not be booked; 84 segment slots of the last ring hold no segment at all.  The row is no multiple
    of 512 samples.  The second ring (segments 64 .. 127: cold, full) takes the IIR wave's lead-in path."""
    n = (1 << 17) + 640
    q = plan(n, 1)
    assert (q["rings"], q["tile_len"], q["tiles_per_ch"]) == (1, 768, 172) and n - 171 * 768 == 384 and n % 512 != 0, q
    pin(monkeypatch)
    u8 = synth.fm_tone(n, seed=2201, deviation=50e3)
    ref, ref_mag, _ = oracle_chain(oracle).accept_stream(u8, 256)
    run_one(capi, u8, 256, ref, ref_mag)


@pytest.mark.parametrize("rings", [None, 3])
def test_channel_ends_and_starts_inside_one_p_wave(capi, monkeypatch, plain_rows, rings):
    """40 channels x 2^13 samples, 11 segments each (the last of 512 samples): a P wave's 16 segments hold one or two channel
    starts - lanes that read the kept tail through the lead-in and move to the call's samples at position 0, beside lanes
    that never do - and as many short last segments.  rings = 3: the three rings of one workgroup side by side."""
    q = plan(N, N_CH, rings=rings)
    assert (q["rings"], q["tile_len"], q["tiles_per_ch"]) == (rings or 1, 768, 11), q
    pin(monkeypatch, rings=rings)
    rows, refs = plain_rows
    eng = capi.Engine(N_CH, block_bytes=256, flags=STREAM)
    eng.set_mode("wbfm")
    check_rows(eng, rows, refs)
    eng.close()


def test_tail_switch_and_carried_state(capi, oracle, monkeypatch):
    """Three consecutive calls of 5, 1 and 7 blocks on one engine: from the second call on the first segment is warm - its
    lead-in is the kept tail's real samples, and the request that follows the lead-in's last must be the call's sample 0."""
    pin(monkeypatch)
    blocks = (5, 1, 7)
    u8 = synth.fm_tone(sum(blocks) * 16384, seed=2202, deviation=60e3)
    chain = oracle_chain(oracle)
    eng = capi.Engine(1, flags=STREAM)
    eng.set_mode("wbfm")
    off = 0
    for k, b in enumerate(blocks):
        part = u8[off:off + b * 32768]
        off += b * 32768
        check_rows(eng, part, [chain.accept_stream(part, 32768)], launches=k + 1)
    eng.close()


def test_chunk_order_with_rotation_selectors_mixed(capi, oracle, monkeypatch):
    """The second case in workgroups of three rings with the selectors +1 / 0 / -1 mixed: the grouped instantiation, which runs
    the P wave's body once per selector."""
    rots = [1, 0, -1, -1, 0, 1, 0, 1] * 5
    q = plan(N, (sum(r == 1 for r in rots), rots.count(0), rots.count(-1)), rings=3)
    assert (q["grouped"], q["rings"], q["tile_len"]) == (1, 3, 768), q
    pin(monkeypatch, rings=3)
    rows = channel_rows()
    eng = capi.Engine(N_CH, block_bytes=256, flags=STREAM)
    eng.set_mode("wbfm")
    for c in range(N_CH):
        eng.set_rotation(rots[c], first=c, n=1)
    check_rows(eng, rows, [oracle_chain(oracle, rotation=rots[c]).accept_stream(rows[c], 256) for c in range(N_CH)])
    eng.close()


def test_chunk_order_in_a_squelch_gated_call(capi, oracle, monkeypatch):
    """The second case in workgroups of three rings, squelch-gated at -60 dBFS: loud blocks (the tone) and quiet ones (silence),
    so the channels' virtual streams have different lengths and the gated instantiation's own addressing runs beside the
    magnitude sums."""
    pin(monkeypatch, rings=3)
    rng = np.random.default_rng(23)
    rows = channel_rows()
    for c in range(N_CH):
        for b0 in rng.integers(0, N // 128 - 6, 4):
            rows[c, 256 * int(b0):256 * (int(b0) + int(rng.integers(2, 6)))] = 128
    chains = [oracle_chain(oracle, threshold=-60) for _ in range(N_CH)]
    refs = [chains[c].accept_stream(rows[c], 256) for c in range(N_CH)]
    assert sum(int(np.count_nonzero(np.asarray(r[2]) == 0)) for r in refs) > N_CH      # the call is gated
    eng = capi.Engine(N_CH, block_bytes=256, flags=STREAM)
    eng.set_mode("wbfm")
    eng.set_squelch(-60)
    check_rows(eng, rows, refs)
    eng.close()
