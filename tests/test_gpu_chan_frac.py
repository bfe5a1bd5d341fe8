"""GPU (MI355X): the fractional-rate channelizer (include/iqdemod.h: "Fractional decimation", captures at P / Q x
256 kS/s) bit for bit against the numpy model of its integer spec (tests/chan_frac_model.py) on the inputs of
tests/chan_frac_cases.py (which tests/test_chan_frac_host.py holds to the mutation proof), across calls, retuning, moving
and reset, its refusals, end to end into the demodulators (against the oracle's chain) and through the iqdemod_wide
tool.  No tolerance anywhere: exact bytes."""
import os
import subprocess

import numpy as np
import pytest

from tests import chan_frac_cases as fc
from tests import chan_frac_model as fm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_NAMES = ["default-%d/%d" % r for r in fc.RATIOS] + [
    "K203-75/8", "K3-17/8", "K1-5/2", "K8187-17/8", "K2047-5/2", "limit-45/4", "limit-25/2", "K33-5/2-300ch",
    "default-75/8-64ch", "default-15/2-1ch", "default-127/2-300ch"]


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def cases(capi):
    got = {c.name: c for c in fc.cases(capi)}
    assert list(got) == CASE_NAMES
    return got


@pytest.mark.parametrize("name", CASE_NAMES)
def test_bit_identical_to_the_model(capi, P, cases, name):
    """One long call, then - after a reset - the same stream in calls of the shortest length (64 P bytes)."""
    c = cases[name]
    want = fm.channelize(c.wide, c.h, c.P, c.Q, c.src, c.inc, c.shift, P)
    assert want.shape == (c.n_ch, c.units * 64 * c.Q)
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, c.P, c.n_ch, n_sources=c.n_src, taps=c.taps, decimation_den=c.Q)
    z.set_channels(0, source=c.src, phase_inc=c.inc, gain_shift=c.shift)
    out = z.run(c.wide)
    bad = [i for i in range(c.n_ch) if not np.array_equal(out[i], want[i])]
    assert not bad, (bad[:8], c.src[bad[0]], c.inc[bad[0]], c.shift[bad[0]],
                     np.nonzero(out[bad[0]] != want[bad[0]])[0][:8])
    assert (out == 0).any() and (out == 255).any()             # both saturations were reached
    z.reset()
    parts = [z.run(c.wide[:, k * c.unit:(k + 1) * c.unit]) for k in range(c.units)]
    assert np.array_equal(np.concatenate(parts, axis=1), want)
    z.close()
    eng.close()


def test_empty_branches_are_0x80_pairs(capi, cases):
    c = cases["K3-17/8"]
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, c.P, c.n_ch, n_sources=c.n_src, taps=c.taps, decimation_den=c.Q)
    z.set_channels(0, source=c.src, phase_inc=c.inc, gain_shift=c.shift)
    out = z.run(c.wide).reshape(c.n_ch, -1, 2)
    r = (np.arange(out.shape[1]) * c.P + c.P - 1) % c.Q
    assert (out[:, r >= 3] == 128).all() and (out[:, r < 3] != 128).any()
    z.close()
    eng.close()


@pytest.mark.parametrize("p,q", [(75, 8), (5, 2), (45, 4)])
def test_uneven_calls_reset_retuning_and_moving(capi, P, p, q):
    rng = np.random.default_rng(5 + p)
    n_src, n_ch = 2, 20
    h = capi.channelizer_default_taps(p, q)
    unit = 64 * p
    cuts = np.cumsum([0, 1, 3, 16, 5, 7])
    wide = np.stack([fc.stream(rng, int(cuts[-1]) * unit, "random") for _ in range(n_src)])
    src, inc, shift = fc.channel_set(rng, n_ch, n_src)
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, p, n_ch, n_sources=n_src, decimation_den=q)
    z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    parts = [z.run(wide[:, a * unit:b * unit]) for a, b in zip(cuts[:-1], cuts[1:])]
    want = fm.channelize(wide, h, p, q, src, inc, shift, P)
    assert np.array_equal(np.concatenate(parts, axis=1), want)

    z.reset()                                            # the stream starts over
    assert np.array_equal(z.run(wide[:, :4 * unit]), want[:, :4 * unit * q // p])

    # retune channels 3..5 after the first 4 units: only they change, and from the call on
    z.reset()
    first = z.run(wide[:, :4 * unit])
    new_inc = np.array([12345678, 2 ** 31 + 7, 99], np.uint64)
    z.set_channels(3, phase_inc=new_inc, gain_shift=[1, 2, 3])
    second = z.run(wide[:, 4 * unit:])
    got = np.concatenate([first, second], axis=1)
    inc2, shift2 = inc.copy(), shift.copy()
    inc2[3:6], shift2[3:6] = new_inc, [1, 2, 3]
    want2 = fm.channelize(wide, h, p, q, src, inc2, shift2, P)
    split = 4 * unit * q // p
    keep = [c for c in range(n_ch) if c not in (3, 4, 5)]
    assert np.array_equal(got[keep], want[keep])
    assert np.array_equal(got[3:6, :split], want[3:6, :split])
    assert np.array_equal(got[3:6, split:], want2[3:6, split:])
    # moving a channel to another source regroups the tiles
    z.set_channels(0, source=[1 - src[0]])
    z.reset()
    src3 = src.copy()
    src3[0] = 1 - src[0]
    assert np.array_equal(z.run(wide), fm.channelize(wide, h, p, q, src3, inc2, shift2, P))
    z.close()
    eng.close()


def test_retuning_on_every_call_host_and_device_forms_agree(capi, P):
    """The device form with a retune before every call and no synchronisation between the calls, against the model and
    against the host form fed the same way."""
    rng = np.random.default_rng(13)
    p, q, n_src, n_ch = 15, 2, 2, 24
    unit = 64 * p
    row = 2 * unit * q // p                               # bytes per channel and call
    h = capi.channelizer_default_taps(p, q)
    wide = np.stack([fc.stream(rng, 12 * unit, "random") for _ in range(n_src)])
    src, inc, shift = fc.channel_set(rng, n_ch, n_src)
    eng = capi.Engine(1)
    za = capi.Channelizer(eng, p, n_ch, n_sources=n_src, decimation_den=q)
    zb = capi.Channelizer(eng, p, n_ch, n_sources=n_src, decimation_den=q)
    for z in (za, zb):
        z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    d_in, d_out = eng.dev_alloc(wide.nbytes), eng.dev_alloc(n_ch * 6 * row)
    want, host = [], []
    for k in range(6):
        part = np.ascontiguousarray(wide[:, 2 * k * unit:2 * (k + 1) * unit])
        eng.dev_upload(d_in + k * part.nbytes, part)
        if k:
            c = int(rng.integers(0, n_ch))
            inc[c] = int(rng.integers(0, 2 ** 32))
            shift[c] = k % 9
            for z in (za, zb):
                z.set_channels(c, phase_inc=[inc[c]], gain_shift=[k % 9])
        za.run_device(d_in + k * part.nbytes, 2 * unit, d_out + k * n_ch * row)
        host.append(zb.run(part))
        full = fm.channelize(wide, h, p, q, src, inc, shift, P)
        want.append(full[:, k * row:(k + 1) * row])
    eng.synchronize()
    for k in range(6):
        got = eng.dev_download(d_out + k * n_ch * row, n_ch * row).reshape(n_ch, -1)
        assert np.array_equal(got, want[k]), k
        assert np.array_equal(host[k], want[k]), k
    eng.dev_free(d_in)
    eng.dev_free(d_out)
    za.close()
    zb.close()
    eng.close()


def test_refusals_queue_nothing(capi):
    eng = capi.Engine(4)
    for p, q in ((75, 3), (75, 16), (75, 5), (6, 4), (12, 8), (74, 8), (3, 2), (15, 8), (129, 2), (513, 8)):
        with pytest.raises(capi.IqdError) as ei:                # bad Q, gcd != 1, P / Q out of range
            capi.Channelizer(eng, p, 4, decimation_den=q)
        assert ei.value.status == -1, (p, q)
    over = np.zeros(2 * 300, np.int16)
    over[0::2] = 27962                                          # branch 0: 300 x 27962 = 8388600, within the limit
    z = capi.Channelizer(eng, 5, 4, taps=over, decimation_den=2)
    z.close()
    over[0] += 8                                                # 8388608: one over
    with pytest.raises(capi.IqdError) as ei:
        capi.Channelizer(eng, 5, 4, taps=over, decimation_den=2)
    assert ei.value.status == -1
    for taps in (np.zeros(0, np.int16), np.ones(2 * 1024 + 1, np.int16), np.array([32640], np.int16)):
        with pytest.raises(capi.IqdError):
            capi.Channelizer(eng, 5, 4, taps=taps, decimation_den=2)
    z = capi.Channelizer(eng, 5, 4, n_sources=2, decimation_den=2)
    quiet = np.full((2, 64 * 5), 128, np.uint8)
    assert np.array_equal(z.run(quiet), np.full((4, 128), 128, np.uint8))
    for n_bytes in (64 * 2, 64 * 6, 64 * 5 + 64, 64 * 5 // 2, 0):      # multiples of 64, not of 64 P
        with pytest.raises(capi.IqdError) as ei:
            z.run(np.zeros((2, n_bytes), np.uint8))
        assert ei.value.status == -1, n_bytes
    with pytest.raises(capi.IqdError) as ei:
        z.follow_scanner(True)
    assert ei.value.status == -1
    z.follow_scanner(False)                                     # nothing to stop: accepted
    with pytest.raises(capi.IqdError):                          # rows of 32768 + 128 bytes: not the engine's block rule
        eng.accept_wideband(z, np.zeros((2, (32768 + 128) * 5 // 2), np.uint8))
    # nothing was queued by the refused calls, and the channelizer is still usable: the stream is where it was
    rng = np.random.default_rng(2)
    wide = rng.integers(0, 256, (2, 64 * 5), dtype=np.uint8)
    P = capi.channelizer_phasor_table()
    both = np.concatenate([quiet, wide], axis=1)
    want = fm.channelize(both, capi.channelizer_default_taps(5, 2), 5, 2, [0] * 4, [0] * 4, [0] * 4, P)
    assert np.array_equal(z.run(wide), want[:, 128:])
    z.close()
    eng.close()


STATIONS = [  # offsets from the capture's centre (2.4 MS/s), each channel placed at station + 64 kHz
    {"offset": -700e3, "kind": "fm", "amplitude": 25.0, "tone": 1000.0, "mode": "fm"},
    {"offset": 250e3, "kind": "am", "amplitude": 25.0, "tone": 700.0, "mode": "am"},
    {"offset": -150e3, "kind": "wbfm", "amplitude": 25.0, "tone": 1500.0, "mode": "wbfm"},
    {"offset": 900e3, "kind": "usb", "amplitude": 25.0, "tone": 1200.0, "mode": "usb"},
]
RATE, P_, Q_ = 2400000.0, 75, 8
BLOCK = 32768 * P_ // Q_                                        # wide bytes of one engine block


def _wide_capture(n_bytes, seed=11):
    from rtlsdrdiags_amd import synth
    return synth.wideband(n_bytes // 2, RATE, STATIONS, seed=seed)


def test_end_to_end_into_the_demodulators(capi, P, oracle):
    wide = _wide_capture(4 * BLOCK)
    n = len(STATIONS)
    eng = capi.Engine(n)
    z = capi.Channelizer(eng, P_, n, decimation_den=Q_)
    offs = [st["offset"] + 64e3 for st in STATIONS]
    z.set_channels(0, source=[0] * n, offset_hz=offs, fs=RATE, gain_shift=[1] * n)   # (amplitude 50: the SSB audio unclipped)
    for c, st in enumerate(STATIONS):
        eng.set_mode(st["mode"], c, 1)
    pcm, cnt, mag, allowed = eng.accept_wideband(z, wide)
    h = capi.channelizer_default_taps(P_, Q_)
    for c, st in enumerate(STATIONS):
        row = fm.channel(wide, h, P_, Q_, capi.phase_inc(offs[c], RATE), 1, P)
        assert len(row) == 4 * 32768
        ch = oracle.chain()
        ch.set_mode(st["mode"])
        ref_pcm, ref_mag, ref_allowed = ch.accept_stream(row)
        assert int(cnt[c]) == len(ref_pcm)
        assert np.array_equal(pcm[c, :cnt[c]], ref_pcm), st
        assert np.array_equal(mag[c], ref_mag) and np.array_equal(allowed[c], ref_allowed)
        x = pcm[c, 512:cnt[c]].astype(np.float64)
        spec = np.abs(np.fft.rfft(x * np.hanning(len(x))))
        f = np.fft.rfftfreq(len(x), 1 / 8000.0)
        spec[f < 200] = 0
        assert abs(f[np.argmax(spec)] - st["tone"]) < 40, (st, f[np.argmax(spec)])
    z.close()
    eng.close()


@pytest.mark.parametrize("blocks,how", [(6, "rate"), (5.5, "rate"), (1.5, "decimation")])
def test_iqdemod_wide_tool_equals_the_python_path(capi, tmp_path, blocks, how):
    """rate=2400000 alone selects 75/8 (or decimation=75/8 says so).  Calls of 4 engine blocks; a capture that ends
    inside a call ends with its whole blocks and then one short block, the rest cut to a multiple of 64 P bytes."""
    n_bytes = int(blocks * BLOCK)
    wide = _wide_capture(n_bytes + (300 if blocks != 6 else 0), seed=12)
    cap = tmp_path / "cap.iq"
    wide.tofile(cap)
    offs = [st["offset"] + 64e3 for st in STATIONS]
    modes = [capi.MODE[st["mode"]] for st in STATIONS]
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_wide")
    args = [tool, "in=%s" % cap, "rate=2400000", "offsets=" + ",".join("%d" % o for o in offs),
            "modes=" + ",".join(map(str, modes)), "gains=3", "out=%s" % (tmp_path / "pcm_%d.s16")]
    if how == "decimation":
        args.insert(2, "decimation=75/8")
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    n = len(STATIONS)
    eng = capi.Engine(n)
    z = capi.Channelizer(eng, P_, n, decimation_den=Q_)
    z.set_channels(0, source=[0] * n, offset_hz=offs, fs=RATE, gain_shift=[3] * n)
    for c, st in enumerate(STATIONS):
        eng.set_mode(st["mode"], c, 1)
    got = [[] for _ in range(n)]
    call = 4 * BLOCK
    for a in range(0, n_bytes, call):
        part = wide[a:min(a + call, n_bytes)]
        whole = len(part) // BLOCK * BLOCK
        for piece in (part[:whole], part[whole:]):
            if len(piece):
                pcm, cnt, _, _ = eng.accept_wideband(z, piece)
                for c in range(n):
                    got[c].append(pcm[c, :cnt[c]])
    for c in range(n):
        pcm_tool = np.fromfile(tmp_path / ("pcm_%d.s16" % c), np.int16)
        assert len(pcm_tool) == n_bytes * Q_ // P_ // 64         # every sample of the capture came out
        assert np.array_equal(pcm_tool, np.concatenate(got[c])), c
    z.close()
    eng.close()


def test_iqdemod_wide_names_the_admissible_rates(tmp_path):
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_wide")
    cap = tmp_path / "cap.iq"
    np.zeros(64, np.uint8).tofile(cap)
    r = subprocess.run([tool, "in=%s" % cap, "rate=2500000", "offsets=0", "modes=2", "out=%s" % (tmp_path / "p_%d.s16")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "256000 P / Q" in r.stderr, r.stderr
