"""GPU (MI355X): the wideband channelizer (include/iqdemod.h: iqd_channelizer_*, iqd_accept_wideband) bit for bit
against the numpy model of its integer spec (tests/chan_model.py), across calls, retuning and reset, at size, end to end
into the demodulators (against the oracle's chain), and through the iqdemod_wide tool."""
import os
import subprocess

import numpy as np
import pytest

from tests import chan_model as cm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCS = [0, 1, 2 ** 31, 2 ** 31 - 1, 2 ** 32 - 1]


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


def _stream(rng, n_bytes, kind):
    """random, or random with full-scale 0x00 / 0xFF / alternating stretches that drive both saturations"""
    u = rng.integers(0, 256, n_bytes, dtype=np.uint8)
    if kind == "rails":
        q = n_bytes // 4 // 2 * 2
        u[q:2 * q] = 0xFF
        u[2 * q:3 * q] = 0x00
        alt = np.tile(np.array([0, 0, 255, 255], np.uint8), q // 4 + 1)[:q]
        u[3 * q:4 * q] = alt
    return u


def _taps(capi, rng, M, K):
    if K == "default":
        return None, capi.channelizer_default_taps(M)
    lim = 32639 if K <= 64 else 8000                  # 256 sum |h| <= 2^31 - 256 for K = 1024
    h = rng.integers(-lim, lim + 1, K).astype(np.int16)
    h[0] = lim                                        # the byte split's extreme
    return h, h


def _channels(rng, n_ch, n_src):
    src = np.arange(n_ch) % n_src
    rng.shuffle(src)
    inc = np.array([INCS[c] if c < len(INCS) else int(rng.integers(0, 2 ** 32)) for c in range(n_ch)], np.uint64)
    shift = np.array([(0, 8)[c % 2] if c < 12 else int(rng.integers(0, 9)) for c in range(n_ch)], np.uint8)
    return src.astype(np.uint32), inc, shift


@pytest.mark.parametrize("M,K,n_src,n_ch", [
    (2, 1, 1, 7), (8, "default", 3, 64), (10, 33, 3, 300), (64, 1024, 1, 1), (64, "default", 3, 7),
    (8, 1024, 1, 7), (2, "default", 1, 64), (10, "default", 1, 1), (8, 33, 3, 7),
    # odd M: windows 2-byte aligned every other output (the v_alignbyte path), A in registers / read per group
    (3, "default", 3, 64), (5, 1024, 1, 7), (7, 33, 3, 300),
])
def test_bit_identical_to_the_model(capi, P, M, K, n_src, n_ch):
    rng = np.random.default_rng(M * 1000 + n_ch)
    taps, h = _taps(capi, rng, M, K)
    n_out = 2048 if M < 64 else 512
    bps = n_out * 2 * M
    wide = np.stack([_stream(rng, bps, "rails" if s % 2 == 0 else "random") for s in range(n_src)])
    src, inc, shift = _channels(rng, n_ch, n_src)
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, M, n_ch, n_sources=n_src, taps=taps)
    z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    out = z.run(wide)
    want = cm.channelize(wide, h, M, src, inc, shift, P)
    bad = [c for c in range(n_ch) if not np.array_equal(out[c], want[c])]
    assert not bad, (bad[:8], src[bad[0]], inc[bad[0]], shift[bad[0]])
    assert (out == 0).any() and (out == 255).any()     # both saturations were reached
    if K not in ("default", 1):                         # and, with random taps, both rails of stage a (sat16)
        a = np.concatenate(cm.channel(wide[src[0]], h, M, int(inc[0]), int(shift[0]), P, stage_a=True))
        assert a.min() == -32768 and a.max() == 32767
    z.close()
    eng.close()


def test_uneven_calls_reset_and_retuning(capi, P):
    rng = np.random.default_rng(5)
    M, n_src, n_ch = 8, 2, 20
    h = capi.channelizer_default_taps(M)
    unit = 64 * M
    cuts = np.cumsum([0, 1, 3, 16, 5, 7])
    wide = np.stack([_stream(rng, int(cuts[-1]) * unit, "random") for _ in range(n_src)])
    src, inc, shift = _channels(rng, n_ch, n_src)
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, M, n_ch, n_sources=n_src)
    z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    parts = [z.run(wide[:, a * unit:b * unit]) for a, b in zip(cuts[:-1], cuts[1:])]
    want = cm.channelize(wide, h, M, src, inc, shift, P)
    assert np.array_equal(np.concatenate(parts, axis=1), want)

    z.reset()                                            # the stream starts over
    assert np.array_equal(z.run(wide[:, :4 * unit]), want[:, :4 * unit // M])

    # retune channels 3..5 after the first 4 units: only they change, and from the call on
    z.reset()
    first = z.run(wide[:, :4 * unit])
    new_inc = np.array([12345678, 2 ** 31 + 7, 99], np.uint64)
    z.set_channels(3, phase_inc=new_inc, gain_shift=[1, 2, 3])
    second = z.run(wide[:, 4 * unit:])
    got = np.concatenate([first, second], axis=1)
    inc2, shift2 = inc.copy(), shift.copy()
    inc2[3:6], shift2[3:6] = new_inc, [1, 2, 3]
    want2 = cm.channelize(wide, h, M, src, inc2, shift2, P)
    split = 4 * unit // M
    keep = [c for c in range(n_ch) if c not in (3, 4, 5)]
    assert np.array_equal(got[keep], want[keep])
    assert np.array_equal(got[3:6, :split], want[3:6, :split])
    assert np.array_equal(got[3:6, split:], want2[3:6, split:])
    # moving a channel to another source regroups the tiles
    z.set_channels(0, source=[1 - src[0]])
    z.reset()
    src3 = src.copy()
    src3[0] = 1 - src[0]
    assert np.array_equal(z.run(wide), cm.channelize(wide, h, M, src3, inc2, shift2, P))
    z.close()
    eng.close()


def test_host_form_equals_device_form(capi):
    rng = np.random.default_rng(9)
    M, n_src, n_ch, bps = 10, 2, 33, 64 * 10 * 40
    wide = rng.integers(0, 256, (n_src, bps), dtype=np.uint8)
    src, inc, shift = _channels(rng, n_ch, n_src)
    eng = capi.Engine(1)
    za, zb = capi.Channelizer(eng, M, n_ch, n_src), capi.Channelizer(eng, M, n_ch, n_src)
    for z in (za, zb):
        z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    host = np.concatenate([za.run(wide[:, :bps // 2]), za.run(wide[:, bps // 2:])], axis=1)
    d_in, d_out = eng.dev_alloc(wide.nbytes), eng.dev_alloc(n_ch * bps // M)
    dev = []
    for half in (wide[:, :bps // 2], wide[:, bps // 2:]):
        eng.dev_upload(d_in, np.ascontiguousarray(half))
        zb.run_device(d_in, bps // 2, d_out)
        eng.synchronize()
        dev.append(eng.dev_download(d_out, n_ch * bps // 2 // M).reshape(n_ch, -1))
    assert np.array_equal(host, np.concatenate(dev, axis=1))
    eng.dev_free(d_in)
    eng.dev_free(d_out)
    za.close()
    zb.close()
    eng.close()


STATIONS = [  # offsets from the capture's centre (2.048 MS/s), each channel placed at station + 64 kHz
    {"offset": -600e3, "kind": "fm", "amplitude": 25.0, "tone": 1000.0, "mode": "fm"},
    {"offset": 250e3, "kind": "am", "amplitude": 25.0, "tone": 700.0, "mode": "am"},
    {"offset": -150e3, "kind": "wbfm", "amplitude": 25.0, "tone": 1500.0, "mode": "wbfm"},
    {"offset": 700e3, "kind": "usb", "amplitude": 25.0, "tone": 1200.0, "mode": "usb"},
]


def _wide_capture(capi, n_bytes, seed=11):
    from rtlsdrdiags_amd import synth
    return synth.wideband(n_bytes // 2, 2048000.0, STATIONS, seed=seed)


def test_end_to_end_into_the_demodulators(capi, P, oracle):
    M, rate = 8, 2048000.0
    wide = _wide_capture(capi, 4 * 32768 * M)
    n = len(STATIONS)
    eng = capi.Engine(n)
    z = capi.Channelizer(eng, M, n)
    offs = [st["offset"] + 64e3 for st in STATIONS]
    z.set_channels(0, source=[0] * n, offset_hz=offs, fs=rate, gain_shift=[2] * n)
    for c, st in enumerate(STATIONS):
        eng.set_mode(st["mode"], c, 1)
    pcm, cnt, mag, allowed = eng.accept_wideband(z, wide)
    h = capi.channelizer_default_taps(M)
    for c, st in enumerate(STATIONS):
        row = cm.channel(wide, h, M, capi.phase_inc(offs[c], rate), 2, P)
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


def test_at_size_4096_channels_from_16_sources(capi, P):
    M, n_src, n_ch, n_out = 8, 16, 4096, 1 << 16
    bps = n_out * 2 * M
    rng = np.random.default_rng(21)
    wide = rng.integers(0, 256, (n_src, bps), dtype=np.uint8)
    src = (np.arange(n_ch) % n_src).astype(np.uint32)
    inc = rng.integers(0, 2 ** 32, n_ch, dtype=np.uint64)
    shift = rng.integers(0, 9, n_ch).astype(np.uint8)
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    d_in, d_out = eng.dev_alloc(wide.nbytes), eng.dev_alloc(n_ch * 2 * n_out)
    eng.dev_upload(d_in, wide)
    z.run_device(d_in, bps, d_out)
    eng.synchronize()
    h = capi.channelizer_default_taps(M)
    for c in rng.choice(n_ch, 40, replace=False):
        row = eng.dev_download(d_out + int(c) * 2 * n_out, 2 * n_out)
        m_a = int(rng.integers(0, n_out - 2048))
        for a, b in ((0, 64), (m_a, m_a + 2048), (n_out - 64, n_out)):
            want = cm.channel(wide[src[c]], h, M, int(inc[c]), int(shift[c]), P, m_range=(a, b))
            assert np.array_equal(row[2 * a:2 * b], want), (c, a)
    eng.dev_free(d_in)
    eng.dev_free(d_out)
    z.close()
    eng.close()


def test_invalid_arguments_are_refused(capi):
    eng = capi.Engine(4)
    for M in (0, 1, 65):
        with pytest.raises(capi.IqdError):
            capi.Channelizer(eng, M, 4)
    for taps in (np.zeros(0, np.int16), np.ones(1025, np.int16), np.array([32640], np.int16),
                 np.array([-32640], np.int16), np.full(300, 30000, np.int16)):
        with pytest.raises(capi.IqdError):
            capi.Channelizer(eng, 8, 4, taps=taps)
    with pytest.raises(capi.IqdError):
        capi.Channelizer(eng, 8, 0)
    z = capi.Channelizer(eng, 8, 4, n_sources=2)
    for bad in (dict(source=[2]), dict(gain_shift=[9])):
        with pytest.raises(capi.IqdError):
            z.set_channels(0, **bad)
    with pytest.raises(capi.IqdError):
        z.set_channels(3, source=[0, 1])                   # past the last channel
    with pytest.raises(capi.IqdError):
        z.run(np.zeros((2, 64 * 8 + 16), np.uint8))       # not a multiple of 64 M
    with pytest.raises(capi.IqdError):
        z.run(np.zeros((2, 0), np.uint8))
    with pytest.raises(capi.IqdError):                     # rows of 32768 + 64 bytes: not the engine's block rule
        eng.accept_wideband(z, np.zeros((2, 8 * (32768 + 64)), np.uint8))
    with pytest.raises(capi.IqdError):                     # channels 2..5 of a 4-channel engine
        eng.accept_wideband(z, np.zeros((2, 8 * 64), np.uint8), first=2)
    # nothing was queued by the refused calls: the stream is where it was
    assert np.array_equal(z.run(np.full((2, 512), 128, np.uint8)), np.full((4, 64), 128, np.uint8))
    z.close()
    eng.close()


@pytest.mark.parametrize("blocks", [6, 5.5, 1.5])
def test_iqdemod_wide_tool_equals_the_python_path(capi, tmp_path, blocks):
    """Calls of 4 engine blocks; a capture that ends inside a call ends with its whole blocks and then one short block
    (5.5 blocks: 4, 1, one half; 1.5: 1, one half), and the 300 bytes past the last 64 M are dropped."""
    M, rate = 8, 2048000.0
    n_bytes = int(blocks * 32768 * M)
    wide = _wide_capture(capi, n_bytes + (300 if blocks != 6 else 0), seed=12)
    cap = tmp_path / "cap.iq"
    wide.tofile(cap)
    offs = [st["offset"] + 64e3 for st in STATIONS]
    modes = [capi.MODE[st["mode"]] for st in STATIONS]
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_wide")
    r = subprocess.run([tool, "in=%s" % cap, "decimation=8", "rate=2048000", "offsets=" + ",".join("%d" % o for o in offs),
                        "modes=" + ",".join(map(str, modes)), "gains=3", "out=%s" % (tmp_path / "pcm_%d.s16")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    n = len(STATIONS)
    eng = capi.Engine(n)
    z = capi.Channelizer(eng, M, n)
    z.set_channels(0, source=[0] * n, offset_hz=offs, fs=rate, gain_shift=[3] * n)
    for c, st in enumerate(STATIONS):
        eng.set_mode(st["mode"], c, 1)
    got = [[] for _ in range(n)]
    call, block = 4 * 32768 * M, 32768 * M
    for a in range(0, n_bytes, call):
        part = wide[a:min(a + call, n_bytes)]
        whole = len(part) // block * block
        for piece in (part[:whole], part[whole:]):
            if len(piece):
                pcm, cnt, _, _ = eng.accept_wideband(z, piece)
                for c in range(n):
                    got[c].append(pcm[c, :cnt[c]])
    for c in range(n):
        pcm_tool = np.fromfile(tmp_path / ("pcm_%d.s16" % c), np.int16)
        assert len(pcm_tool) == n_bytes // M // 64               # every sample of the capture came out
        assert np.array_equal(pcm_tool, np.concatenate(got[c])), c
    z.close()
    eng.close()


def test_retuning_on_every_call(capi, P):
    """A host that retunes between calls (a scanner): each call's new taps reach the next run, uploads queued behind
    the work before them, across both staging slots."""
    rng = np.random.default_rng(13)
    M, n_src, n_ch, unit = 5, 2, 24, 64 * 5
    h = capi.channelizer_default_taps(M)
    wide = np.stack([_stream(rng, 12 * unit, "random") for _ in range(n_src)])
    src, inc, shift = _channels(rng, n_ch, n_src)
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, M, n_ch, n_sources=n_src)
    z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    d_in, d_out = eng.dev_alloc(wide.nbytes), eng.dev_alloc(n_ch * 12 * unit // M)
    got, want = [], []
    for k in range(6):                                     # device form, no synchronisation between the calls
        part = np.ascontiguousarray(wide[:, 2 * k * unit:2 * (k + 1) * unit])
        eng.dev_upload(d_in + k * part.nbytes, part)
        if k:
            c = int(rng.integers(0, n_ch))
            inc[c] = int(rng.integers(0, 2 ** 32))
            z.set_channels(c, phase_inc=[inc[c]], gain_shift=[k % 9])
            shift[c] = k % 9
        z.run_device(d_in + k * part.nbytes, 2 * unit, d_out + k * n_ch * 2 * unit // M)
        full = cm.channelize(wide, h, M, src, inc, shift, P)
        want.append(full[:, 2 * k * unit // M:2 * (k + 1) * unit // M])
    eng.synchronize()
    for k in range(6):
        got = eng.dev_download(d_out + k * n_ch * 2 * unit // M, n_ch * 2 * unit // M).reshape(n_ch, -1)
        assert np.array_equal(got, want[k]), k
    eng.dev_free(d_in)
    eng.dev_free(d_out)
    z.close()
    eng.close()


def test_engine_closed_before_its_channelizer(capi):
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, 8, 3)
    assert z.run(np.full(512, 128, np.uint8)).shape == (3, 64)
    eng.close()                                            # destroys the channelizer first
    z.close()
    del z
