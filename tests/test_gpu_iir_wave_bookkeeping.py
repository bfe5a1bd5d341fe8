"""GPU (MI355X): the per-piece bookkeeping of the WBFM streaming kernel's IIR waves (iqd_stream.hip: st_iir_wave, st_iir_piece,
st_iir_window, st_iir_lead_in) - the two ring polls on the scalar unit through an address kept in a vector register, the ring
chunks read through addresses pinned in registers, and the de-emphasis input sums formed from the chunks (u0, u2, u1, u3) with
one packed addition per chunk (st_iir_sums).  The fast piece (rings of cold full segments, behind st_iir_lead_in), the general piece
(warm first segments, short last segments, the keeper of a channel's restart state) and the lead-in share all of it.

Every case pins the streaming path (IQD_F_WBFM_STREAM), holds the planner to the shape it relies on, compares PCM, counts,
magnitudes and squelch flags with the oracle sample for sample and asserts that no hand-off needed a repair (a wrong boundary
record shows in the 21 PCM samples behind a boundary, or as a repair).  Small shapes: the planner gives them 768-sample segments,
whose restart record sits at position 0, the fast loop's first window; the 1024-sample case has it eight pieces into the loop.

More than one round can be pinned only with more channels than a round has segment slots, and then every channel is ONE
segment - a warm one, so such a launch runs the general piece only (a ring of cold full segments needs a channel of more than 64
segments, which the planner fits into one round by making them longer).  That case is here: the piece counters of both hand-overs
run on from round to round."""
import numpy as np
import pytest

from rtlsdrdiags_amd import synth
from test_gpu_audio_wave import STREAM, oracle_chain, pin, plan

pytestmark = pytest.mark.gpu

N_CH, N = 40, 1 << 13


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


def channel_rows(n_ch=N_CH):
    """n_ch channels x 2^13 samples, each with its own data."""
    return np.stack([synth.fm_tone(N, seed=2400 + c, deviation=11e3 + 1400 * c, amplitude=24.0 + 2 * (c % 45)) for c in range(n_ch)])


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


def one_row(capi, oracle, u8, block_bytes):
    ref, ref_mag, ref_allowed = oracle_chain(oracle).accept_stream(u8, block_bytes)
    eng = capi.Engine(1, block_bytes=block_bytes, flags=STREAM)
    eng.set_mode("wbfm")
    check_rows(eng, u8, [(ref, ref_mag, ref_allowed)])
    eng.close()


def test_fast_ring_beside_a_general_one(capi, oracle, monkeypatch):
    """One channel of 2^17 + 640 samples with 256-byte blocks: 172 segments of 768 samples, the last of 384, one ring per
    workgroup.  Ring 0 holds the warm first segment and runs the general piece from its first piece on; ring 1 (segments 64 .. 127)
    is cold and full: the lead-in, then 24 fast pieces with the record (position 0) and the first 48 samples' values in the first
    two; the last ring holds the short segment and 84 empty slots."""
    n = (1 << 17) + 640
    q = plan(n, 1)
    assert (q["rings"], q["tile_len"], q["tiles_per_ch"], q["rounds"]) == (1, 768, 172, 1) and n - 171 * 768 == 384, q
    pin(monkeypatch)
    one_row(capi, oracle, synth.fm_tone(n, seed=2301, deviation=50e3), 256)


def test_record_inside_the_fast_loop(capi, oracle, monkeypatch):
    """One channel of 2^17 samples on two workgroups of one ring: 128 segments of 1024 samples.  The second ring is fast, and
    its restart record (position 256) is taken eight pieces into the fast loop, not in its first window."""
    n = 1 << 17
    q = plan(n, 1, rings=1, wgs=2)
    assert (q["rings"], q["tile_len"], q["tiles_per_ch"], q["grid"], q["rounds"]) == (1, 1024, 128, 2, 1), q
    pin(monkeypatch, rings=1, wgs=2)
    one_row(capi, oracle, synth.fm_tone(n, seed=2302, deviation=45e3), 32768)


@pytest.mark.parametrize("rings", [None, 3])
def test_three_rings_side_by_side(capi, monkeypatch, plain_rows, rings):
    """40 channels x 2^13 samples, 11 segments each (the last of 512 samples): channel starts, short last segments and the
    keepers of the restart state before them fall at different lanes of one IIR wave.  rings = 3: the three rings of one
    workgroup side by side."""
    q = plan(N, N_CH, rings=rings)
    assert (q["rings"], q["tile_len"], q["tiles_per_ch"], q["rounds"]) == (rings or 1, 768, 11, 1), q
    pin(monkeypatch, rings=rings)
    rows, refs = plain_rows
    eng = capi.Engine(N_CH, block_bytes=256, flags=STREAM)
    eng.set_mode("wbfm")
    check_rows(eng, rows, refs)
    eng.close()


def test_carried_state_across_calls(capi, oracle, monkeypatch):
    """Three consecutive calls of 5, 1 and 7 blocks of 32 768 bytes on one engine, the restart state carried from call to call.
    The calls are 107, 22 and 150 segments of 768 samples on rings of 64:
    the second call's single block is ONE ring, with the warm first segment in it - the general piece only; the first and the
    third have fast rings behind the first."""
    pin(monkeypatch)
    blocks = (5, 1, 7)
    for b, tiles in zip(blocks, (107, 22, 150)):
        q = plan(b * 16384, 1)
        assert (q["rings"], q["tile_len"], q["tiles_per_ch"], q["rounds"]) == (1, 768, tiles, 1), q
    u8 = synth.fm_tone(sum(blocks) * 16384, seed=2303, deviation=60e3)
    chain = oracle_chain(oracle)
    eng = capi.Engine(1, flags=STREAM)
    eng.set_mode("wbfm")
    off = 0
    for k, b in enumerate(blocks):
        part = u8[off:off + b * 32768]
        off += b * 32768
        check_rows(eng, part, [chain.accept_stream(part, 32768)], launches=k + 1)
    eng.close()


def test_squelch_gated(capi, oracle, monkeypatch):
    """The 40 channels in workgroups of three rings, squelch-gated at -60 dBFS with silent stretches written into the rows: the
    gated instantiations compile the same loops, and the channels' virtual streams have different lengths."""
    q = plan(N, N_CH, rings=3, gated=True)
    assert (q["rings"], q["tile_len"]) == (3, 768), q
    pin(monkeypatch, rings=3)
    rng = np.random.default_rng(24)
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


def test_grouped_rotation_selectors(capi, oracle, monkeypatch):
    """The 40 channels in workgroups of three rings with the selectors +1 / 0 / -1 mixed: the grouped instantiation (ROT = 2),
    whose segment ids are padded per group - rings hold ids that are no segment."""
    rots = [1, 0, -1, -1, 0, 1, 0, 1] * 5
    q = plan(N, (sum(r == 1 for r in rots), rots.count(0), rots.count(-1)), rings=3)
    assert (q["grouped"], q["rings"], q["tile_len"], q["rounds"]) == (1, 3, 768, 1), q
    pin(monkeypatch, rings=3)
    rows = channel_rows()
    eng = capi.Engine(N_CH, block_bytes=256, flags=STREAM)
    eng.set_mode("wbfm")
    for c in range(N_CH):
        eng.set_rotation(rots[c], first=c, n=1)
    check_rows(eng, rows, [oracle_chain(oracle, rotation=rots[c]).accept_stream(rows[c], 256) for c in range(N_CH)])
    eng.close()


def test_two_rounds_of_one_ring(capi, oracle, monkeypatch):
    """70 channels x 2^13 on ONE workgroup of one ring: every channel is one 8192-sample segment, 64 of them in the first round and
    6 in the second.  Both piece counters (ring pieces read, pairs handed to the audio wave) count on across the rounds."""
    n_ch = 70
    q = plan(N, n_ch, rings=1, wgs=1)
    assert (q["rings"], q["tile_len"], q["tiles_per_ch"], q["grid"], q["rounds"]) == (1, 8192, 1, 1, 2), q
    pin(monkeypatch, rings=1, wgs=1)
    rows = channel_rows(n_ch)
    eng = capi.Engine(n_ch, block_bytes=256, flags=STREAM)
    eng.set_mode("wbfm")
    check_rows(eng, rows, [oracle_chain(oracle).accept_stream(rows[c], 256) for c in range(n_ch)])
    eng.close()
