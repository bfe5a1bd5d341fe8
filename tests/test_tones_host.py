"""CPU tier of the PCM tone bank (include/iqdemod_tones.h): the corpus of tests/tones_cases.py proven against the defects of
tests/tones_model.py; the CTCSS defaults with the library's phasor table; the host-only helpers against Python integers; the
add-on header against the binding's own prototype table and struct mirrors; the chain test's signal on the oracle alone.
No GPU: the library is loaded for its host-only functions."""
import re

import numpy as np
import pytest

from rtlsdrdiags_amd import capi, tones
from tests import addon_checks as ac
from tests import tones_cases as tc
from tests import tones_model as tm
from tests.test_abi_layout import mirror_layout


@pytest.fixture(scope="module")
def phasor():
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def cases(phasor):
    return tc.build(phasor)


# ---- the corpus against the model's defects ----

def test_every_defect_changes_a_case_and_every_case_names_its_blind_spots(cases, phasor):
    assert len({c.name for c in cases}) == len(cases) and set(tc.BLIND) == {c.name for c in cases}
    seen = set()
    for c in cases:
        assert c.blind <= set(tm.DEFECTS), c.name
        want = tc.run_model(c, phasor)
        blind = {d for d in tm.DEFECTS if tc.same(want, tc.run_model(c, phasor, d))}
        assert blind == c.blind, (c.name, sorted(blind ^ c.blind))
        seen |= set(tm.DEFECTS) - blind
    assert seen == set(tm.DEFECTS)


def test_the_corpus_covers_the_shapes(cases, phasor):
    assert {c.L for c in cases} == {32, 64, 96, 4096, 8192}
    assert {len(c.incs) for c in cases} >= {1, 2, 15, 16, 17, 50, 64}
    assert {c.C for c in cases} >= {1, 15, 16, 17, 65}
    rel = set()                                                  # n of a call relative to its L
    for c in cases:
        runs = [s for s in c.steps if s[0] == "run"]
        rel |= {("0", "1", "L-1", "L", "L+1", "3L+5")[(0, 1, c.L - 1, c.L, c.L + 1, 3 * c.L + 5).index(s[2])] for s in runs
                if s[2] in (0, 1, c.L - 1, c.L, c.L + 1, 3 * c.L + 5)}
        assert all(s[1].shape[1] > s[2] for s in runs), c.name   # row_stride > n
    assert rel == {"0", "1", "L-1", "L", "L+1", "3L+5"}
    counted = [s for c in cases for s in c.steps if s[0] == "run" and s[3] is not None]
    assert any((s[3] == 0).any() and (s[3] > s[2]).any() and len(set(s[3].tolist())) > 2 for s in counted)
    flags = {int(f) for c in cases for r in tc.run_model(c, phasor)[0] for f in np.unique(r[1]["flags"])}
    assert flags == {0, tm.F_OPENED, tm.F_CLOSED, tm.F_OPENED | tm.F_CLOSED}
    # frames that straddle two and three calls
    c = next(c for c in cases if c.name == "l32_t17_c17_cuts")
    assert [s[2] for s in c.steps][:4] == [0, 1, 31, 32]


def test_a_frame_of_the_bound_case_reaches_two_to_the_43(cases, phasor):
    c = next(c for c in cases if c.name == "l8192_bound_t64")
    coef = tm.coefficients(c.L, c.incs[:1], c.window, phasor)
    A = int(abs(coef[0, 0].sum() * -32768))
    assert 2 ** 42 < A < 2 ** 44
    frames = tc.run_model(c, phasor)[0][0][1]
    assert int(frames[0, 0]["p_best"]) * c.thresholds["ratio_q8"] >= 2 ** 64 and frames[0, 0]["best"] == 0 and frames[0, 0]["second"] == 1


# ---- the defaults of set=ctcss ----

def clean_tone(freq_mhz, n, amp=1000):
    return np.rint(amp * np.cos(2 * np.pi * (freq_mhz / 1000.0) * np.arange(n) / tc.PCM_RATE)).astype(np.int16)


def test_every_ctcss_tone_is_best_at_4096_by_a_ratio_of_two(phasor):
    assert tones.ctcss_mhz().tolist() == tc.CTCSS_MHZ and len(tc.CTCSS_MHZ) == 50
    incs = [tones.phase_inc(f, tc.PCM_RATE) for f in tc.CTCSS_MHZ]
    assert incs == [tm.phase_inc(f, tc.PCM_RATE) for f in tc.CTCSS_MHZ]
    m = tm.Model(50, 4096, incs, phasor, **{k: v for k, v in tones.CTCSS_DEFAULTS.items() if k != "frame_len"})
    x = np.stack([clean_tone(f, 2 * 4096) for f in tc.CTCSS_MHZ])
    nf, frames, power = m.run(x, 2 * 4096)
    ratios = {}
    for t, f in enumerate(tc.CTCSS_MHZ):
        assert nf[t] == 2 and frames[t, 0]["best"] == t, (f, frames[t, 0])
        ratios[f] = int(frames[t, 0]["p_best"]) / int(frames[t, 0]["p_second"])
        assert ratios[f] >= 2.0, (f, ratios[f])
        assert frames[t, 1]["tone"] == t and frames[t, 1]["flags"] == tm.F_OPENED and frames[t, 0]["tone"] == -1, f   # open = 2
    print("smallest p_best / p_second at L = 4096: %.2f at %.1f Hz" % (min(ratios.values()), min(ratios, key=ratios.get) / 1000.0))
    assert 6.0 < min(ratios.values()) < 9.0          # 7.3 with a rounded cosine for the table; the closest pair is 67.0 / 69.3


def test_at_2048_the_closest_pair_is_too_close_for_a_ratio_of_two(phasor):
    incs = [tm.phase_inc(f, tc.PCM_RATE) for f in tc.CTCSS_MHZ]
    m = tm.Model(50, 2048, incs, phasor)
    _, frames, _ = m.run(np.stack([clean_tone(f, 2048) for f in tc.CTCSS_MHZ]), 2048)
    assert min(int(r["p_best"]) / int(r["p_second"]) for r in frames[:, 0]) < 2.0


# ---- host-only helpers ----

def test_phase_inc_against_python_integers():
    for f, r in [(0, 1), (0, 8000), (1, 8000), (67000, 8000), (254100, 8000), (3999999, 8000), (499, 1), (1, 0xffffffff),
                 (500 * 0xffffffff - 1, 0xffffffff), (1750000, 48000), (123456789, 250000)]:
        assert tones.phase_inc(f, r) == tm.phase_inc(f, r) < 2 ** 32, (f, r)
    for f, r in [(4000000, 8000), (500, 1), (0, 0), (1, 0), (500 * 0xffffffff, 0xffffffff), (2 ** 64 - 1, 8000)]:
        with pytest.raises(capi.IqdError):
            tones.phase_inc(f, r)
    with pytest.raises(capi.IqdError):
        tones.phase_inc(2 ** 64, 8000)
    assert tones._lib().iqd_tones_phase_inc(1000, 8000, None) == -1


def test_default_window_and_tone_lists(phasor):
    for L in (32, 64, 96, 4096, 8192):
        w = tones.default_window(L)
        assert np.array_equal(w, tm.default_window(L, phasor)) and w.min() >= 0 and w.max() <= 16383
    n = np.arange(8192)
    assert np.array_equal(tones.default_window(8192), (32767 - phasor[(2 * n + 1) * 2048 // 8192, 0].astype(np.int64)) >> 2)
    for L in (0, 31, 33, 16, 8224, 2 ** 32):
        with pytest.raises(capi.IqdError):
            tones.default_window(L)
    assert tones.dtmf_mhz().tolist() == [697000, 770000, 852000, 941000, 1209000, 1336000, 1477000, 1633000]
    assert tones._lib().iqd_tones_ctcss(None) == -1 and tones._lib().iqd_tones_dtmf(None) == -1
    assert tones._lib().iqd_tones_max_frames(None, 100) == 0


# ---- the add-on header against the binding ----

def test_the_add_on_table_is_the_add_on_header():
    ac.check_table_is_header("tones", tones, 11)
    assert re.search(r"#define IQD_TONES_ABI_VERSION (\d+)", open(ac.header_path("tones")).read()).group(1) == str(tones.ABI_VERSION)
    assert (tones.F_OPENED, tones.F_CLOSED, tones.NONE) == (tm.F_OPENED, tm.F_CLOSED, tm.NONE) == (1, 2, 0xffffffff)


def test_the_library_exports_the_add_on_and_binds_it_from_its_own_table():
    ac.check_library_binding(tones)


MIRROR = {"iqd_tones_config": tones.TonesConfig, "iqd_tones_frame": tones.TONES_FRAME, "iqd_tones_state": tones.TonesState}


def test_every_struct_of_the_add_on_matches_its_mirror(tmp_path):
    """a stand-alone C program, compiled with the address and undefined-behaviour sanitizers, prints the layouts"""
    compiled = ac.compiled_layouts("tones", MIRROR, tmp_path)
    assert mirror_layout(tm.FRAME) == mirror_layout(tones.TONES_FRAME) and compiled["iqd_tones_frame"][0] == 40
    assert compiled["iqd_tones_config"][0] == 72 and compiled["iqd_tones_state"][0] == 32


# ---- the chain test's signal: the oracle's PCM alone must name the injected tone ----

def test_the_oracle_pcm_of_the_chain_signal_names_the_injected_tone(oracle, phasor):
    chain = oracle.chain()
    chain.set_mode("fm")
    pcm, _, _ = chain.accept_stream(tc.chain_iq())
    assert len(pcm) == tc.CHAIN_FRAMES * 4096
    incs = [tm.phase_inc(f, tc.PCM_RATE) for f in tc.CTCSS_MHZ]
    m = tm.Model(1, 4096, incs, phasor, **{k: v for k, v in tones.CTCSS_DEFAULTS.items() if k != "frame_len"})
    nf, frames, _ = m.run(pcm[None, :], len(pcm))
    print([(int(r["best"]), int(r["p_best"]) / max(int(r["p_second"]), 1), int(r["tone"]), int(r["flags"])) for r in frames[0]])
    assert nf[0] == tc.CHAIN_FRAMES and (frames[0]["best"] == tc.CHAIN_TONE).all()
    assert frames[0, 0]["tone"] == -1 and (frames[0, 1:]["tone"] == tc.CHAIN_TONE).all() and frames[0, 1]["flags"] == tm.F_OPENED
    assert all(256 * int(r["p_best"]) >= 1024 * int(r["p_second"]) for r in frames[0])       # twice the default ratio to spare
