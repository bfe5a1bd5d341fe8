"""CPU tier of the PCM packet decoder (include/iqdemod_fsk.h): the corpus of tests/fsk_cases.py proven against the defects of
tests/fsk_model.py; the shapes and events the corpus must cover; the host-only helpers against Python integers; the add-on
header against the binding's own prototype table and struct mirrors; the chain test's signal on the oracle alone.
No GPU: the library is loaded for its host-only functions."""
import re

import numpy as np
import pytest

from rtlsdrdiags_amd import capi, fsk
from tests import addon_checks as ac
from tests import fsk_cases as fc
from tests import fsk_model as fm
from tests.test_abi_layout import mirror_layout


@pytest.fixture(scope="module")
def phasor():
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def cases(phasor):
    return fc.build(phasor)


@pytest.fixture(scope="module")
def results(cases, phasor):
    return {c.name: fc.run_model(c, phasor) for c in cases}


# ---- the corpus against the model's defects ----

def test_every_defect_changes_a_case_and_every_case_names_its_blind_spots(cases, results, phasor):
    """all 16 seeded defects change some output of some case: none had to be left out"""
    assert len({c.name for c in cases}) == len(cases) and set(fc.BLIND) == {c.name for c in cases}
    assert len(fm.DEFECTS) == 16
    seen = set()
    for c in cases:
        assert c.blind <= set(fm.DEFECTS), c.name
        want = results[c.name]
        blind = {d for d in fm.DEFECTS if fc.same(want, fc.run_model(c, phasor, d))}
        assert blind == c.blind, (c.name, sorted(blind ^ c.blind))
        seen |= set(fm.DEFECTS) - blind
    assert seen == set(fm.DEFECTS)


def test_the_corpus_covers_the_shapes(cases, results):
    assert {c.cfg["corr_len"] for c in cases} == {2, 7, 8, 63, 64}
    assert {c.C for c in cases} >= {1, 2, 63, 64, 65}
    assert {c.cfg["loop_shift"] for c in cases} >= {1, 8} and {c.cfg["flags"] for c in cases} == {0, fm.NRZI}
    assert {c.cfg["baud_inc"] for c in cases} >= {1 << 20, (1 << 31) - 1}
    ns = set()
    for c in cases:
        runs = [s for s in c.steps if s[0] == "run"]
        W = c.cfg["corr_len"]
        ns |= {"W-1" for s in runs if s[2] == W - 1} | {"W" for s in runs if s[2] == W} | {s[2] for s in runs}
        assert all(s[1].shape[1] > s[2] for s in runs), c.name   # row_stride > n
    assert ns >= {0, 1, 31, 32, 33, 64, 65, "W-1", "W"} and any(isinstance(n, int) and 300 <= n <= 900 for n in ns)
    counted = [s for c in cases for s in c.steps if s[0] == "run" and s[3] is not None]
    assert any((s[3] == 0).any() and (s[3] > s[2]).any() and len(set(s[3].tolist())) > 2 for s in counted)
    assert any(s[0] == "reset" for c in cases for s in c.steps)


def test_the_corpus_covers_the_framing_events(cases, results):
    found = {name: fc.frames_found(r) for name, r in results.items()}
    # a cut at every bit: one frame, found whole, on both channels; every call is one bit long
    c = next(c for c in cases if c.name == "t8_every_bit_a_call")
    assert [(ch, p) for ch, _, p in found[c.name]] == [(0, b"\xff\x3e\xa7"), (1, b"\xff\x3e\xa7")] and {s[2] for s in c.steps} == {8}
    # shared flags, a shared zero: every frame found; one frame over three calls (it ends in the third), two closing in one
    assert [p for ch, _, p in found["t8_shared_flags"] if ch == 0] == [b"\x01\x02\x03\x04", b"\xf0", b"\x7e\x7e"]
    assert [p for ch, _, p in found["t8_shared_flags"] if ch == 1] == [b"\xaa", b"\x55\x00\xff", b"\x1f\xf8\x00"]
    per_call = [r[2].tolist() for r in results["t8_shared_flags"][0]]
    assert per_call[:2] == [[0, 0], [0, 1]] and per_call[2][0] == 1 and max(per_call[3]) >= 2, per_call
    # min_len and max_len stand, below and above are dropped; the bad FCS is counted once; the abort loses its frame only
    assert [p for _, _, p in found["t8_lengths_bad_fcs_abort"]] == [b"\x33\x44\x55", b"\x01\x02\x03\x04\x05\x06", b"\x99\x88\x77\x66"]
    st = results["t8_lengths_bad_fcs_abort"][1][0]
    assert st["bad_fcs"] == 1 and st["frames_total"] == 3
    # NRZI off, before and after the reset, on nearly every channel (loop_shift 1 under noise loses a few)
    assert 120 <= len(found["w7_c63_nrzi_off_small_n"]) <= 2 * 63 and {p for _, _, p in found["w7_c63_nrzi_off_small_n"]} == {b"\xde\xad\xbe\xef"}
    assert len(found["afsk1200_noise"]) == 2 and len(found["afsk1200_noise"][0][2]) == 20
    # a channel whose count is 0 keeps its state in that call
    assert results["t8_c64_counts"][0][0][0][0] == 0


def test_the_bound_case_reaches_the_accumulators_limits(cases, phasor):
    c = next(c for c in cases if c.name == "w64_bound_soft_zero")
    m = c.model(phasor)
    assert np.abs(m.coef[0]).min() == 127 and np.abs(m.coef[2]).min() == 127 and not m.coef[1].any() and not m.coef[3].any()
    peak = 64 * 127 * 32768
    assert 2 ** 27 < peak < 2 ** 28 and 2 ** 55 < peak * peak < 2 ** 56     # one tone of the two: |soft| < 2^57 with room
    x = np.concatenate([s[1][0, :s[2]] for s in c.steps]).astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(np.concatenate([np.zeros(63, np.int64), x]), 64)
    acc = win @ m.coef.T
    soft = [int(a) ** 2 + int(b) ** 2 - int(e) ** 2 - int(f) ** 2 for a, b, e, f in acc.tolist()]
    assert max(soft) == peak * peak and min(soft) < -(2 ** 55) and 0 in soft


# ---- host-only helpers ----

def test_phase_inc_against_python_integers():
    for f, r in [(0, 1), (0, 8000), (1, 8000), (1200000, 8000), (2200000, 8000), (3999999, 8000), (499, 1), (1, 0xffffffff),
                 (500 * 0xffffffff - 1, 0xffffffff), (1200000, 48000), (123456789, 250000)]:
        assert fsk.phase_inc(f, r) == fm.phase_inc(f, r) < 2 ** 32, (f, r)
    for f, r in [(4000000, 8000), (500, 1), (0, 0), (1, 0), (500 * 0xffffffff, 0xffffffff), (2 ** 64 - 1, 8000)]:
        with pytest.raises(capi.IqdError):
            fsk.phase_inc(f, r)
    with pytest.raises(capi.IqdError):
        fsk.phase_inc(2 ** 64, 8000)
    assert fsk._lib().iqd_fsk_phase_inc(1000, 8000, None) == -1


def test_afsk1200_and_the_size_functions_without_an_object():
    for rate in (8000, 11025, 22050, 48000):
        assert fsk.afsk1200(rate) == fm.afsk1200(rate), rate
    assert fsk.afsk1200(8000)["baud_inc"] == 644245094 and fsk.afsk1200(8000)["flags"] == fsk.NRZI == fm.NRZI
    for rate in (0, 2400, 4400, 2 ** 32):           # 1200 baud needs more than 2400 Hz, 2200 Hz more than 4400 Hz
        with pytest.raises(capi.IqdError):
            fsk.afsk1200(rate)
    lib = fsk._lib()
    assert lib.iqd_fsk_afsk1200(8000, None) == -1
    assert lib.iqd_fsk_max_frames(None, 100) == lib.iqd_fsk_max_bit_words(None, 100) == lib.iqd_fsk_max_bytes(None, 100) == 0


def test_the_models_sizes_follow_the_header(phasor):
    m = fm.Model(1, phasor, **fm.afsk1200(8000))
    b = m.b
    assert m.maxbits(0) == 0 and (m.max_frames(0), m.max_bit_words(0), m.max_bytes(0)) == (0, 0, 0)
    mb = (2048 * (b + (b >> 3))) // 2 ** 32 + 1
    assert m.maxbits(2048) == mb == 346
    assert (m.max_frames(2048), m.max_bit_words(2048), m.max_bytes(2048)) == (mb // 144 + 1, (mb + 31) // 32, (512 + mb // 8 + 15) // 16 * 16)


# ---- the add-on header against the binding ----

def test_the_add_on_table_is_the_add_on_header():
    ac.check_table_is_header("fsk", fsk, 11)
    text = open(ac.header_path("fsk")).read()
    assert re.search(r"#define IQD_FSK_ABI_VERSION (\d+)", text).group(1) == str(fsk.ABI_VERSION)
    assert re.search(r"#define IQD_FSK_NRZI (\d+)u", text).group(1) == str(fsk.NRZI)


def test_the_library_exports_the_add_on_and_binds_it_from_its_own_table():
    ac.check_library_binding(fsk)


MIRROR = {"iqd_fsk_config": fsk.FskConfig, "iqd_fsk_frame": fsk.FSK_FRAME, "iqd_fsk_state": fsk.FskState}


def test_every_struct_of_the_add_on_matches_its_mirror(tmp_path):
    """a stand-alone C program, compiled with the address and undefined-behaviour sanitizers, prints the layouts"""
    compiled = ac.compiled_layouts("fsk", MIRROR, tmp_path)
    assert mirror_layout(fm.FRAME) == mirror_layout(fsk.FSK_FRAME) and compiled["iqd_fsk_frame"][0] == 24
    assert compiled["iqd_fsk_config"][0] == 64 and compiled["iqd_fsk_state"][0] == 40


# ---- the chain test's signal: the oracle's FM PCM alone must decode to the payload ----

def test_the_oracle_pcm_of_the_chain_signal_decodes_to_the_payload(oracle, phasor):
    chain = oracle.chain()
    chain.set_mode("fm")
    iq = fc.chain_iq()
    assert len(iq) % 32768 == 0
    pcm, _, _ = chain.accept_stream(iq)
    m = fm.Model(1, phasor, **fm.afsk1200(8000))
    nb, _, nf, frames, data = m.run(pcm[None, :], len(pcm))
    print("bits", int(nb[0]), "frames", int(nf[0]), "bad_fcs", m.state(0)["bad_fcs"])
    assert nf[0] == 1 and m.state(0)["bad_fcs"] == 0
    r = frames[0, 0]
    assert bytes(data[0, r["offset"]:r["offset"] + r["len"]]) == fc.chain_payload() and r["len"] == 40
