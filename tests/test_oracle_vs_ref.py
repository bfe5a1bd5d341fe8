"""CPU: the oracle against the reference on fresh random inputs.  The reference's results for every case are recorded in
tests/golden/oracle_vs_ref.npz (tests/golden/make_golden.py), so the comparison runs wherever the suite runs; where the live
reference is built (oracle/_ref) each case also runs there and must still give exactly the record."""
import os

import numpy as np
import pytest

from rtlsdrdiags_amd import synth

MODES = ["am", "fm", "wbfm", "lsb", "usb"]
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_ref.npz")


@pytest.fixture(scope="module")
def recorded():
    """recorded(key, run) -> the reference's arrays for one case; run(new_chain) computes them with new_chain(agc=False)."""
    from oracle import bindings as B
    store = np.load(RECORD)
    ref = B.Reference() if B.have_ref() else None

    def get(key, run):
        want = [store["%s__%d" % (key, i)] for i in range(int(store[key + "__n"]))]
        if ref is not None:
            live = run(lambda agc=False: ref.chain(agc=agc))
            assert len(live) == len(want) and all(np.array_equal(a, b) for a, b in zip(live, want)), key
        return want
    return get


def oracle_run(oracle, run):
    return run(lambda agc=False: oracle.chain())


def check(want, got):
    assert len(want) == len(got)
    for k, (a, b) in enumerate(zip(want, got)):
        assert np.array_equal(a, b), k


def random_streams(new_chain, mode, seed):
    rng = np.random.default_rng(seed)
    kind = seed % 2
    u8 = synth.fm_tone(3 * 16384, seed=seed, amplitude=float(rng.uniform(20, 120)),
                       deviation=float(rng.uniform(2e3, 7e4))) if kind else synth.white_u8(3 * 16384, seed)
    gain = {"am": 1, "fm": 2, "wbfm": 3, "lsb": 4, "usb": 4}[mode]
    g = float(rng.uniform(0.2, 3.0)) * {1: 300, 2: 10185.9, 3: 40743.7, 4: 300}[gain]
    c = new_chain()
    c.set_mode(mode)
    c.set_gain(gain, g)
    return list(c.accept_stream(u8))


def squelch_thresholds(new_chain):
    amps = [1, 30, 30, 1, 1, 80, 1, 120, 127, 0, 5, 5]
    u8 = synth.stepped_amplitude(amps, block_samples=1024, seed=9)
    out = []
    for thr in (-200, -60, -45, -30, -24, 0):
        for gain_db in (0, 24, 40):
            c = new_chain()
            c.set_mode("am")
            c.set_squelch(thr)
            c.set_rx_gain_db(gain_db)
            out.extend(c.accept_stream(u8, 2048))
    new_chain().set_rx_gain_db(24)
    return out


def reset_semantics(new_chain):
    u8 = synth.fm_tone(2 * 16384, seed=12)
    out = []
    for mode in MODES:
        c = new_chain()
        c.set_mode(mode)
        a, _, _ = c.accept_stream(u8[:32768])
        c.reset()
        b, _, _ = c.accept_stream(u8[32768:])
        out.append(np.concatenate([a, b]))
    return out


def demod_level_entry(new_chain):
    rng = np.random.default_rng(5)
    s8 = rng.integers(-128, 128, 32768).astype(np.int8)
    return [new_chain().demod_accept(mode, s8) for mode in MODES]


def agc_random_command_scripts(new_chain, seed):
    codes, values = A.random_script(seed)
    return list(A.replay(new_chain(agc=True), codes, values))


def agc_inside_random_streams(new_chain, seed):
    rng = np.random.default_rng(seed)
    amps = [int(a) for a in np.clip(np.repeat(rng.integers(1, 128, 10), rng.integers(1, 6, 10)), 0, 127)]
    u8 = synth.stepped_amplitude(amps, block_samples=1024, seed=seed)
    cfg = dict(mode=["am", "fm", "wbfm", "lsb"][seed % 4], threshold=int(rng.integers(-60, -40)),
               type=int(seed % 2), alpha=float(rng.choice([0.2, 0.5, 0.8])), deadband=int(rng.integers(0, 4)),
               blanking=int(rng.integers(0, 4)), operating_point=int(rng.integers(-20, -5)))
    c = new_chain(agc=True)
    A.configure(c, cfg)
    return list(A.stream(c, u8, 2048))


def gain_changes_between_blocks(new_chain, mode):
    u8 = synth.fm_tone(6 * 16384, seed=44)
    which = {"am": 1, "fm": 2, "wbfm": 3, "usb": 4}[mode]
    base = {1: 300.0, 2: 10185.9, 3: 40743.7, 4: 300.0}[which]
    c = new_chain()
    c.set_mode(mode)
    parts = []
    for k, g in enumerate([1.0, 0.25, 0.25, 3.0, 0.01, 1.0]):
        c.set_gain(which, base * g)
        parts.append(c.accept_stream(u8[k * 32768:(k + 1) * 32768])[0])
    return [np.concatenate(parts)]


# (key, case, arguments) of every recorded case: the record holds <key>__n and <key>__<i> for each
CASES = ([("random_streams-%s-%d" % (m, s), random_streams, (m, s)) for s in (101, 102) for m in MODES] +
         [("squelch_thresholds", squelch_thresholds, ()), ("reset_semantics", reset_semantics, ()),
          ("demod_level_entry", demod_level_entry, ())] +
         [("agc_random_command_scripts-%d" % s, agc_random_command_scripts, (s,)) for s in range(100, 140)] +
         [("agc_inside_random_streams-%d" % s, agc_inside_random_streams, (s,)) for s in (31, 32, 33, 34)] +
         [("gain_changes_between_blocks-%s" % m, gain_changes_between_blocks, (m,)) for m in ("fm", "wbfm", "am", "usb")])


def run_case(oracle, recorded, key, case, *args):
    check(recorded(key, lambda new_chain: case(new_chain, *args)), oracle_run(oracle, lambda new_chain: case(new_chain, *args)))


@pytest.mark.parametrize("seed", [101, 102])
@pytest.mark.parametrize("mode", MODES)
def test_random_streams(oracle, recorded, mode, seed):
    run_case(oracle, recorded, "random_streams-%s-%d" % (mode, seed), random_streams, mode, seed)


def test_squelch_thresholds(oracle, recorded):
    run_case(oracle, recorded, "squelch_thresholds", squelch_thresholds)


def test_reset_semantics(oracle, recorded):
    """resetDemodulator(): WBFM keeps its de-emphasis state (WbFmDemodulator.cc:304-320)."""
    run_case(oracle, recorded, "reset_semantics", reset_semantics)


def test_demod_level_entry(oracle, recorded):
    run_case(oracle, recorded, "demod_level_entry", demod_level_entry)


# ---- AutomaticGainControl ---------------------------------------------------------------------------
import agc_script as A  # noqa: E402


@pytest.mark.parametrize("seed", range(100, 140))
def test_agc_random_command_scripts(oracle, recorded, seed):
    run_case(oracle, recorded, "agc_random_command_scripts-%d" % seed, agc_random_command_scripts, seed)


@pytest.mark.parametrize("seed", [31, 32, 33, 34])
def test_agc_inside_random_streams(oracle, recorded, seed):
    run_case(oracle, recorded, "agc_inside_random_streams-%d" % seed, agc_inside_random_streams, seed)


@pytest.mark.parametrize("mode", ["fm", "wbfm", "am", "usb"])
def test_gain_changes_between_blocks(oracle, recorded, mode):
    """setDemodulatorGain at run time: the demodulators' decimator histories keep what the old gain produced."""
    run_case(oracle, recorded, "gain_changes_between_blocks-%s" % mode, gain_changes_between_blocks, mode)


# ---- the survey's own anchors: yoyo.iq through the boundary harness --------------------------------
YOYO = "/root/reference/demodulatorResearch/yoyo.iq"
YOYO_MD5 = {"am": "1105b36160c8", "fm": "312e523797d5", "wbfm": "0ba876d90f05", "lsb": "acc98d5d0f75", "usb": "02ccbc29006c"}


@pytest.mark.skipif(not os.path.exists(YOYO), reason="build container only: the reference's capture is not copied (SURVEY 8(c))")
@pytest.mark.parametrize("mode", MODES)
def test_survey_md5_anchors_on_the_reference_capture(oracle, reference, mode):
    """The survey's independent harness fed yoyo.iq (+128) through IqDataProcessor::acceptIqData and recorded md5(PCM) per
    mode; oracle/_ref (the unmodified reference compiled in place) and the oracle restatement must both land on them.
    Ties oracle/_ref to a harness this builder did not write; the capture itself stays where it is."""
    import hashlib
    s8 = np.fromfile(YOYO, dtype=np.int8)
    assert len(s8) == 2 * (1 << 20)
    u8 = (s8.astype(np.int16) + 128).astype(np.uint8)
    for which in (reference, oracle):
        c = which.chain()
        c.set_mode(mode)
        pcm, _, _ = c.accept_stream(u8)
        assert pcm.nbytes == 65536
        assert hashlib.md5(pcm.tobytes()).hexdigest().startswith(YOYO_MD5[mode]), (mode, which)


REF_DEMOD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "ref_demod")


@pytest.mark.skipif(not os.path.exists(REF_DEMOD), reason="build container only: oracle/_ref/ref_demod is the reference's demod.cc compiled in place")
@pytest.mark.parametrize("dtype", [1, 2, 3, 4, 5])
def test_demod_tool_fixture_is_the_reference_programs_output(dtype):
    import subprocess
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demod_tool.npz"))
    r = subprocess.run([REF_DEMOD, "-d", str(dtype)], input=g["iq_s8"].tobytes(), stdout=subprocess.PIPE, check=True)
    assert np.array_equal(np.frombuffer(r.stdout, dtype=np.int16), g["pcm_%d" % dtype])


def test_the_hot_path_pin_shares_no_binary_with_the_agc_test_double():
    """oracle/_ref/libiqd_ref.so holds the reference's hot path and the two externals only; the AGC, the
    scanner and the harness' test double of their owner (class Radio's five accessors) live in libiqd_ref_agc.so, which only
    the (f)-2 / (f)-3 pins load."""
    import subprocess
    from oracle import bindings as B
    if not B.have_ref():
        pytest.skip("oracle/_ref not built")
    hot = subprocess.run(["nm", "-D", "--defined-only", B.REF_SO], capture_output=True, text=True, check=True).stdout
    agc = subprocess.run(["nm", "-D", "--defined-only", B.REF_AGC_SO], capture_output=True, text=True, check=True).stdout
    for needle in ("5Radio", "AutomaticGainControl", "FrequencyScanner", "ref_agc_", "ref_scanner_"):
        assert needle not in hot, needle
        assert needle in agc, needle
    assert "radio_adjustableReceiveGainInDb" in hot and "nprintf" in hot and "ref_accept_stream" in hot
