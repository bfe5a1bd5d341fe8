"""GPU (MI355X): the channelizer on signed 8-bit and 16-bit captures (include/iqdemod.h: "Signed captures") bit for bit
against the numpy model of its integer spec (tests/chan_fmt_model.py) on the inputs of tests/chan_fmt_cases.py (which
tests/test_chan_fmt_host.py holds to the mutation proof), against the U8 channelizer on the same signal, across calls,
retuning, moving and reset, its refusals, end to end into the demodulators (against the oracle's chains) and through the
iqdemod_wide tool.  No tolerance anywhere: exact bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import chan_fmt_cases as fc
from tests import chan_fmt_model as fm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_NAMES = fc.case_names()


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
    """One long call in the host form, then - after a reset - the same stream in the device form, cut as the case says: a
    chain of calls of the shortest length, then the rest."""
    c = cases[name]
    want = fm.channelize(c.wide, c.fmt, c.h, c.M, c.src, c.inc, c.shift, P)
    B = fm.RAIL_BYTES[c.fmt]
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, c.M, len(c.src), n_sources=c.n_src, taps=c.taps, sample_format=c.fmt)
    z.set_channels(0, source=c.src, phase_inc=c.inc, gain_shift=c.shift)
    out = z.run(c.wide)
    bad = [i for i in range(len(c.src)) if not np.array_equal(out[i], want[i])]
    assert not bad, (bad[:8], c.src[bad[0]], c.inc[bad[0]], c.shift[bad[0]], np.nonzero(out[bad[0]] != want[bad[0]])[0][:8])
    z.reset()
    n_ch = len(c.src)
    d_in, d_out = eng.dev_alloc(c.wide.nbytes), eng.dev_alloc(want.size)
    at, spans = 0, []
    for n in c.calls:                                            # every call's bytes and rows at their own place
        part = np.ascontiguousarray(c.wide[:, 2 * at:2 * (at + n)])
        eng.dev_upload(d_in + 2 * at * B * c.n_src, part)
        z.run_device(d_in + 2 * at * B * c.n_src, 2 * n * B, d_out + 2 * (at // c.M) * n_ch)
        spans.append((2 * (at // c.M), 2 * (n // c.M)))
        at += n
    eng.synchronize()
    for o, r in spans:
        got = eng.dev_download(d_out + o * n_ch, r * n_ch).reshape(n_ch, r)
        assert np.array_equal(got, want[:, o:o + r]), (name, o)
    eng.dev_free(d_in)
    eng.dev_free(d_out)
    z.close()
    eng.close()


@pytest.mark.parametrize("M,n_ch", [(7, 20), (8, 70)])
def test_the_same_signal_in_three_formats_gives_the_same_rows(capi, M, n_ch):
    """The existing U8 channelizer on u8, against S8 on u8 ^ 0x80 and S16 on 256 (u8 - 128): byte-identical rows, call by
    call.  This does not rest on the new model."""
    rng = np.random.default_rng(40 + M)
    n_src, unit = 2, 64 * M
    cuts = np.cumsum([0, 1, 40, 2, 9])                           # (M = 7, S16: 40 units = 1280 outputs, two windows)
    u8 = rng.integers(0, 256, (n_src, int(cuts[-1]) * unit), dtype=np.uint8)
    u8[:, :8] = [0, 255, 255, 0, 0, 0, 255, 255]
    src, inc, shift = fc.channel_set(rng, n_ch, [0, 1])
    eng = capi.Engine(1)
    rows = {}
    for fmt in ("u8", "s8", "s16"):
        z = capi.Channelizer(eng, M, n_ch, n_sources=n_src, sample_format=fmt)
        z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
        w = u8 if fmt == "u8" else fm.from_u8(u8, fmt)
        B = w.dtype.itemsize
        rows[fmt] = np.concatenate([z.run(w[:, a * unit:b * unit]) for a, b in zip(cuts[:-1], cuts[1:])], axis=1)
        assert rows[fmt].shape == (n_ch, u8.shape[1] // M) and B == z.rail_bytes
        z.close()
    assert (rows["u8"] == 0).any() and (rows["u8"] == 255).any() and len(np.unique(rows["u8"])) > 200
    assert np.array_equal(rows["s8"], rows["u8"])
    assert np.array_equal(rows["s16"], rows["u8"])
    eng.close()


@pytest.mark.parametrize("fmt", ["s8", "s16"])
def test_uneven_calls_reset_retuning_and_moving(capi, P, fmt):
    rng = np.random.default_rng(5)
    M, n_src, n_ch = 8, 2, 20
    h = capi.channelizer_default_taps(M)
    unit = 32 * M                                                # samples of the shortest call
    cuts = np.cumsum([0, 1, 3, 16, 5, 7])
    wide = np.stack([fc.full_random(rng, int(cuts[-1]) * unit, fmt) for _ in range(n_src)])
    src, inc, shift = fc.channel_set(rng, n_ch, [0, 1])
    eng = capi.Engine(1)
    z = capi.Channelizer(eng, M, n_ch, n_sources=n_src, sample_format=fmt)
    z.set_channels(0, source=src, phase_inc=inc, gain_shift=shift)
    parts = [z.run(wide[:, 2 * a * unit:2 * b * unit]) for a, b in zip(cuts[:-1], cuts[1:])]
    want = fm.channelize(wide, fmt, h, M, src, inc, shift, P)
    assert np.array_equal(np.concatenate(parts, axis=1), want)

    z.reset()                                                    # the stream starts over
    assert np.array_equal(z.run(wide[:, :2 * 4 * unit]), want[:, :2 * 4 * 32])

    # retune channels 3..5 after the first 4 units: only they change, and from the call on
    z.reset()
    first = z.run(wide[:, :2 * 4 * unit])
    new_inc = np.array([12345678, 2 ** 31 + 7, 99], np.uint64)
    z.set_channels(3, phase_inc=new_inc, gain_shift=[1, 2, 3])
    second = z.run(wide[:, 2 * 4 * unit:])
    got = np.concatenate([first, second], axis=1)
    inc2, shift2 = inc.copy(), shift.copy()
    inc2[3:6], shift2[3:6] = new_inc, [1, 2, 3]
    want2 = fm.channelize(wide, fmt, h, M, src, inc2, shift2, P)
    split = 2 * 4 * 32
    keep = [c for c in range(n_ch) if c not in (3, 4, 5)]
    assert np.array_equal(got[keep], want[keep])
    assert np.array_equal(got[3:6, :split], want[3:6, :split])
    assert np.array_equal(got[3:6, split:], want2[3:6, split:])
    # moving a channel to another source regroups the tiles
    z.set_channels(0, source=[1 - src[0]])
    z.reset()
    src3 = src.copy()
    src3[0] = 1 - src[0]
    assert np.array_equal(z.run(wide), fm.channelize(wide, fmt, h, M, src3, inc2, shift2, P))
    z.close()
    eng.close()


@pytest.mark.parametrize("fmt", ["s8", "s16"])
def test_refusals_name_the_format_and_queue_nothing(capi, P, fmt):
    eng = capi.Engine(4)
    name = "IQD_WIDE_" + fmt.upper()
    with pytest.raises(capi.IqdError) as ei:                     # no fractional rate on a signed capture
        capi.Channelizer(eng, 75, 4, decimation_den=8, sample_format=fmt)
    assert ei.value.status == -1 and name in str(ei.value)
    cfg = capi.ChannelizerConfig(1, 4, 8, 0, None, 1, 3)         # sample_format 3; and a reserved field that is not 0
    h = C.c_void_p()
    assert capi._lib().iqd_channelizer_create(eng._h, C.byref(cfg), C.byref(h)) == -1
    cfg = capi.ChannelizerConfig(1, 4, 8, 0, None, 1, capi.SAMPLE_FORMAT[fmt][0], (C.c_uint32 * 2)(0, 1))
    assert capi._lib().iqd_channelizer_create(eng._h, C.byref(cfg), C.byref(h)) == -1
    with pytest.raises(ValueError):
        capi.Channelizer(eng, 8, 4, sample_format="cf32")

    M, B = 8, fm.RAIL_BYTES[fmt]
    z = capi.Channelizer(eng, M, 4, n_sources=2, sample_format=fmt)
    quiet = np.zeros((2, 2 * 32 * M), fm.DTYPE[fmt])
    assert np.array_equal(z.run(quiet), np.full((4, 64), 128, np.uint8))
    with pytest.raises(capi.IqdError) as ei:
        z.follow_scanner(True)
    assert ei.value.status == -1 and name in str(ei.value)
    z.follow_scanner(False)                                      # nothing to stop: accepted
    with pytest.raises(capi.IqdError) as ei:
        z.set_survey(phase_inc=[0, 1 << 20])
    assert ei.value.status == -1 and name in str(ei.value)
    z.set_survey(phase_inc=[])                                   # no points: accepted
    for samples in (16 * M, 48 * M, 32 * M + 32, 0):             # not a multiple of 64 M B bytes
        with pytest.raises(capi.IqdError) as ei:
            z.run(np.zeros((2, 2 * samples), fm.DTYPE[fmt]))
        assert ei.value.status == -1, samples
    for wrong in (np.uint8, np.int16 if fmt == "s8" else np.int8):   # another format's array: refused before the C call
        with pytest.raises(TypeError):
            z.run(np.zeros((2, 2 * 32 * M * B), wrong))
        with pytest.raises(TypeError):
            eng.accept_wideband(z, np.zeros((2, 2 * 32 * M * B), wrong))
    zu = capi.Channelizer(eng, M, 4, n_sources=2)
    for wrong in (np.int8, np.int16):
        with pytest.raises(TypeError):
            zu.run(np.zeros((2, 64 * M), wrong))
    zu.close()
    with pytest.raises(capi.IqdError):                           # rows of 32768 + 128 bytes: not the engine's block rule
        eng.accept_wideband(z, np.zeros((2, (32768 + 128) * M), fm.DTYPE[fmt]))
    # nothing was queued by the refused calls, and the channelizer is still usable: the stream is where it was
    rng = np.random.default_rng(2)
    wide = np.stack([fc.full_random(rng, 32 * M, fmt) for _ in range(2)])
    both = np.concatenate([quiet, wide], axis=1)
    want = fm.channelize(both, fmt, capi.channelizer_default_taps(M), M, [0] * 4, [0] * 4, [0] * 4, P)
    assert np.array_equal(z.run(wide), want[:, 64:])
    z.close()
    eng.close()


STATIONS = [  # offsets from the capture's centre (2.048 MS/s), each channel placed at station + 64 kHz
    {"offset": -700e3, "kind": "fm", "amplitude": 25.0, "tone": 1000.0, "mode": "fm"},
    {"offset": 250e3, "kind": "am", "amplitude": 25.0, "tone": 700.0, "mode": "am"},
]
RATE, M_ = 2048000.0, 8
BLOCK = 32768 * M_                                               # wide samples x 2 of one engine block: bytes at B = 1


def _capture(n_pairs, fmt, seed=11):
    """a capture of n_pairs samples of the format: the synthetic stations at about a tenth of full scale; on S16 the low
    byte is live (the 8-bit capture times 97, plus noise)"""
    from rtlsdrdiags_amd import synth
    u8 = synth.wideband(n_pairs, RATE, STATIONS, seed=seed)
    if fmt == "s8":
        return (u8 ^ 0x80).view(np.int8)
    rng = np.random.default_rng(seed)
    return ((u8.astype(np.int64) - 128) * 97 + rng.integers(-40, 41, len(u8))).astype(fm.DTYPE["s16"])


def test_s16_capture_end_to_end_into_fm_and_am(capi, P, oracle):
    wide = _capture(2 * BLOCK // 2, "s16")
    assert len(np.unique(wide & 0xff)) == 256                    # the low byte carries signal
    n = len(STATIONS)
    eng = capi.Engine(n)
    z = capi.Channelizer(eng, M_, n, sample_format="s16")
    offs = [st["offset"] + 64e3 for st in STATIONS]
    z.set_channels(0, source=[0] * n, offset_hz=offs, fs=RATE, gain_shift=[3] * n)
    for c, st in enumerate(STATIONS):
        eng.set_mode(st["mode"], c, 1)
    pcm, cnt, mag, allowed = eng.accept_wideband(z, wide)
    h = capi.channelizer_default_taps(M_)
    rows = fm.channelize(wide, "s16", h, M_, [0] * n, [capi.phase_inc(o, RATE) for o in offs], [3] * n, P)
    assert rows.shape == (n, 2 * 32768)
    for c, st in enumerate(STATIONS):
        ch = oracle.chain()
        ch.set_mode(st["mode"])
        ref_pcm, ref_mag, ref_allowed = ch.accept_stream(rows[c])
        assert int(cnt[c]) == len(ref_pcm)
        assert np.array_equal(pcm[c, :cnt[c]], ref_pcm), st
        assert np.array_equal(mag[c], ref_mag) and np.array_equal(allowed[c], ref_allowed)
        x = pcm[c, 256:cnt[c]].astype(np.float64)
        spec = np.abs(np.fft.rfft(x * np.hanning(len(x))))
        f = np.fft.rfftfreq(len(x), 1 / 8000.0)
        spec[f < 200] = 0
        assert abs(f[np.argmax(spec)] - st["tone"]) < 60, (st, f[np.argmax(spec)])
    z.close()
    eng.close()


@pytest.mark.parametrize("fmt,blocks", [("s16", 5.5), ("s8", 1.5)])
def test_iqdemod_wide_tool_equals_the_python_path(capi, tmp_path, fmt, blocks):
    """Calls of 4 engine blocks; a capture that ends inside a call ends with its whole blocks and then one short block, the
    rest cut to a multiple of 64 M B bytes."""
    B = fm.RAIL_BYTES[fmt]
    n_pairs = int(blocks * BLOCK) // 2                           # whole samples the tool uses
    wide = _capture(n_pairs + 75, fmt, seed=12)                  # (and a rest it drops)
    cap = tmp_path / "cap.iq"
    wide.tofile(cap)
    offs = [st["offset"] + 64e3 for st in STATIONS]
    modes = [capi.MODE[st["mode"]] for st in STATIONS]
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_wide")
    args = [tool, "in=%s" % cap, "rate=2048000", "format=" + fmt, "offsets=" + ",".join("%d" % o for o in offs),
            "modes=" + ",".join(map(str, modes)), "gains=3", "out=%s" % (tmp_path / "pcm_%d.s16")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    n = len(STATIONS)
    eng = capi.Engine(n)
    z = capi.Channelizer(eng, M_, n, sample_format=fmt)
    z.set_channels(0, source=[0] * n, offset_hz=offs, fs=RATE, gain_shift=[3] * n)
    for c, st in enumerate(STATIONS):
        eng.set_mode(st["mode"], c, 1)
    got = [[] for _ in range(n)]
    call, n_el = 4 * BLOCK, 2 * n_pairs                          # in array elements (one rail each)
    for a in range(0, n_el, call):
        part = wide[a:min(a + call, n_el)]
        whole = len(part) // BLOCK * BLOCK
        for piece in (part[:whole], part[whole:]):
            if len(piece):
                pcm, cnt, _, _ = eng.accept_wideband(z, piece)
                for c in range(n):
                    got[c].append(pcm[c, :cnt[c]])
    for c in range(n):
        pcm_tool = np.fromfile(tmp_path / ("pcm_%d.s16" % c), np.int16)
        assert len(pcm_tool) == n_el // M_ // 64                 # every sample of the capture came out
        assert np.array_equal(pcm_tool, np.concatenate(got[c])), c
    z.close()
    eng.close()


@pytest.mark.parametrize("extra,what", [(["survey=0,12500,4", "surveylog=x.log"], "survey="),
                                        (["scan=100000000,101000000,25000"], "scan="),
                                        (["decimation=75/8"], "a fractional rate")])
def test_iqdemod_wide_refuses_what_is_not_built(tmp_path, extra, what):
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_wide")
    cap = tmp_path / "cap.iq"
    np.zeros(64, np.int16).tofile(cap)
    r = subprocess.run([tool, "in=%s" % cap, "rate=2048000", "format=s16", "offsets=0", "modes=2",
                        "out=%s" % (tmp_path / "p_%d.s16")] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "format=s16" in r.stderr and what in r.stderr, r.stderr
    assert len(r.stderr.strip().splitlines()) == 1
    r = subprocess.run([tool, "in=%s" % cap, "rate=2048000", "format=cf32", "offsets=0", "modes=2",
                        "out=%s" % (tmp_path / "p_%d.s16")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "u8, s8 or s16" in r.stderr
