"""GPU (MI355X): gain-following wideband channels (include/iqdemod.h: iqd_channelizer_follow_gain) bit for bit against
the model (tests/chan_gain_model.py: the oracle chain's IF gain picks each block's gain in dB) on the inputs of
tests/chan_gain_cases.py, against fixed channels through chz_kernel where the gain is a multiple of 6 dB, across call
boundaries, beside fixed and scanner-following channels, through every refusal, as a closed loop, and through iqdemod_wide."""
import os
import subprocess

import numpy as np
import pytest

from tests import chan_gain_cases as gc
from tests import chan_gain_model as gm
from tests import chan_model as cm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def cases(capi):
    return {c.name: c for c in gc.cases(capi)}


_TRUTH = {}


def truth(oracle, P, case, c):
    """the model's run of channel c of a case, computed once: (rows, pcm, magnitude, allowed, gains), a list per call"""
    key = (case.name, int(c))
    if key not in _TRUTH:
        _TRUTH[key] = gc.run_model(gm, oracle, case, P, int(c))
    return _TRUTH[key]


def _engine(capi, case, n=None):
    eng = capi.Engine(len(case.src) if n is None else n, block_bytes=case.bb)
    eng.set_mode("fm")
    eng.set_squelch(case.threshold)
    if case.agc is not None:
        eng.agc_set_type(case.agc)
        eng.agc_enable(True)
    eng.set_gain_trace(True)
    return eng


def _channelizer(capi, eng, case, follow=True):
    z = capi.Channelizer(eng, case.M, len(case.src), case.n_src, taps=case.taps)
    z.set_channels(0, source=case.src, phase_inc=case.inc, gain_shift=case.shift)
    for c in np.nonzero(case.follow)[0] if follow else []:
        z.follow_gain(True, int(c), 1)
    return z


def _dev_call(eng, z, wide, bb, first=0):
    """iqd_accept_wideband_device -> rows, pcm, counts, magnitude, allowed"""
    n, bps = z.n_channels, wide.shape[1]
    row = bps // z.decimation
    nblk = row // bb if row % bb == 0 else 1
    d_w, d_r = eng.dev_alloc(wide.nbytes), eng.dev_alloc(n * row)
    d_p, d_c = eng.dev_alloc(n * row // 64 * 2), eng.dev_alloc(4 * n)
    d_m, d_a = eng.dev_alloc(4 * n * nblk), eng.dev_alloc(n * nblk)
    eng.dev_upload(d_w, np.ascontiguousarray(wide))
    eng.accept_wideband_device(z, d_w, bps, d_r, d_p, d_c, d_m, d_a, first=first)
    eng.synchronize()
    out = (eng.dev_download(d_r, n * row).reshape(n, row),
           eng.dev_download(d_p, n * row // 64 * 2, np.int16).reshape(n, -1),
           eng.dev_download(d_c, 4 * n, np.uint32), eng.dev_download(d_m, 4 * n * nblk, np.uint32).reshape(n, nblk),
           eng.dev_download(d_a, n * nblk).reshape(n, nblk))
    for d in (d_w, d_r, d_p, d_c, d_m, d_a):
        eng.dev_free(d)
    return out


def _pieces(case):
    at = 0
    for k, row in enumerate(case.calls):
        yield k, row, case.wide[:, at * case.M:(at + row) * case.M]
        at += row


def _set_manual(eng, case, k):
    for c, g in case.manual.get(k, {}).items():
        eng.set_rx_gain_db(g, c, 1)


def _check_call(oracle, P, case, k, got_rows, pcm, cnt, mag, alw, gtrace, m_at):
    """one call's results against the model: following channels in full, fixed ones by their rows"""
    n_out = case.calls[k] // 2
    for c in range(len(case.src)):
        if not case.follow[c]:
            if got_rows is not None:
                want = cm.channel(case.wide[case.src[c]], case.h, case.M, int(case.inc[c]), int(case.shift[c]), P,
                                  m_range=(m_at, m_at + n_out))
                assert np.array_equal(got_rows[c], want), (case.name, k, c)
            continue
        r, p, mg, al, g = (x[k] for x in truth(oracle, P, case, c))
        if got_rows is not None:
            assert np.array_equal(got_rows[c], r), (case.name, k, c)
        assert cnt[c] == len(p) and np.array_equal(pcm[c, :cnt[c]], p), (case.name, k, c)
        assert np.array_equal(mag[c], mg) and np.array_equal(alw[c], al), (case.name, k, c, mag[c], mg)
        assert np.array_equal(gtrace[c], g), (case.name, k, c, gtrace[c], g)


@pytest.mark.parametrize("name", gc.case_names())
def test_bit_identical_to_the_model(capi, P, oracle, cases, name):
    """rows, PCM, magnitudes, flags and the gain trace of every call, through the device form and the host form"""
    case = cases[name]
    for dev in (True, False):
        eng = _engine(capi, case)
        z = _channelizer(capi, eng, case)
        m_at, moved = 0, False
        for k, row, piece in _pieces(case):
            _set_manual(eng, case, k)
            nblk = max(1, row // case.bb)
            if dev:
                rows, pcm, cnt, mag, alw = _dev_call(eng, z, piece, case.bb)
            else:
                rows = None
                pcm, cnt, mag, alw = eng.accept_wideband(z, piece)
            gt = eng.gain_trace(nblk)
            _check_call(oracle, P, case, k, rows, pcm, cnt, mag, alw, gt, m_at)
            moved = moved or any(len(set(gt[c].tolist())) > 1 for c in np.nonzero(case.follow)[0])
            m_at += row // 2
        assert moved == (case.agc is not None)       # an AGC moved the gain inside a call
        z.close()
        eng.close()


@pytest.mark.parametrize("n_ch,n_src", [(18, 1), (4096, 16)])
def test_gain_of_6_L_equals_the_fixed_channel_with_shift_L(capi, n_ch, n_src):
    """An oracle that does not rest on the model: AGC off, manual gains 6 L - a following channel's rows are the fixed
    channel's with gain_shift = L through chz_kernel.  4096 channels: walker workgroups of more than one tile."""
    M, bb, nblk = 8, 256, 4
    rng = np.random.default_rng(n_ch)
    wide = rng.integers(0, 256, (n_src, 2 * nblk * bb * M), dtype=np.uint8)
    src = (np.arange(n_ch) % n_src).astype(np.uint32)
    inc = rng.integers(0, 2 ** 32, n_ch, dtype=np.uint64)
    L = (np.arange(n_ch) % 9).astype(np.uint8)
    eng = capi.Engine(n_ch, block_bytes=bb)
    eng.set_mode("fm")
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=src, phase_inc=inc, gain_shift=(8 - L))   # (ignored while the channels follow)
    z.follow_gain(True)
    e2 = capi.Engine(1)
    z2 = capi.Channelizer(e2, M, n_ch, n_src)
    z2.set_channels(0, source=src, phase_inc=inc, gain_shift=L)
    for c in range(n_ch):
        eng.set_rx_gain_db(6 * int(L[c]), c, 1)
    for half in range(2):
        piece = wide[:, half * nblk * bb * M:(half + 1) * nblk * bb * M]
        got = _dev_call(eng, z, piece, bb)[0]
        assert np.array_equal(got, z2.run(piece)), half
    z.close(); z2.close()
    eng.close(); e2.close()


def test_one_call_of_twelve_blocks_or_twelve_calls_of_one(capi, cases):
    case = cases["M8-7ch-lowpass"]
    res = []
    for step in (12, 1):
        eng = _engine(capi, case)
        z = _channelizer(capi, eng, case)
        rows, pcm, gt = [], [[] for _ in case.src], []
        for b in range(0, 12, step):
            got = _dev_call(eng, z, case.wide[:, b * case.bb * case.M:(b + step) * case.bb * case.M], case.bb)
            rows.append(got[0])
            for c in range(len(case.src)):
                pcm[c].append(got[1][c, :got[2][c]])
            gt.append(eng.gain_trace(step))
        res.append((np.concatenate(rows, 1), [np.concatenate(p) for p in pcm], np.concatenate(gt, 1)))
        z.close()
        eng.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][2], res[1][2])
    assert all(np.array_equal(a, b) for a, b in zip(res[0][1], res[1][1]))
    assert any(len(set(g.tolist())) > 2 for g in res[0][2])


def test_fixed_and_scanner_following_channels_are_what_they_are_without_a_gain_follower(capi):
    M, bb, nblk, n = 8, 1024, 6, 20
    fs, base = 256000 * M, 1_700_000_000
    wide = gc.capture(M, nblk * bb // 2 * M, 77, sigma=1.0)[None]
    rng = np.random.default_rng(5)
    inc = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    inc[12:] = [gc.inc_of(gc.CARRIERS[c % 3][0]) for c in range(8)]
    res = []
    for with_gain in (True, False):
        eng = capi.Engine(n, block_bytes=bb)
        eng.set_mode("fm")
        eng.set_squelch(-50)
        eng.agc_set_type(1)
        eng.agc_enable(True)
        eng.set_gain_trace(True)
        for c in range(6, 12):                       # scanners over the carriers
            start = base + int((-0.3 + 0.02 * c) * fs)
            eng.scanner_set_parameters(start, start + int(0.6 * fs), int(0.05 * fs), first=c, n=1)
            eng.scanner_start(True, c, 1)
        z = capi.Channelizer(eng, M, n)
        z.set_channels(0, source=[0] * n, phase_inc=inc, gain_shift=[c % 4 for c in range(n)])
        z.set_source_frequency([base])
        z.follow_scanner(True, 6, 6)
        if with_gain:
            z.follow_gain(True, 12, 8)
        out = []
        for half in range(2):
            piece = wide[:, half * nblk * bb * M // 2:(half + 1) * nblk * bb * M // 2]
            got = _dev_call(eng, z, piece, bb)
            out.append(got + (eng.frequency_trace(nblk // 2),))
        res.append(out)
        z.close()
        eng.close()
    for a, b in zip(*res):
        assert np.array_equal(a[0][:12], b[0][:12]) and np.array_equal(a[2][:12], b[2][:12])
        assert all(np.array_equal(a[1][c, :a[2][c]], b[1][c, :b[2][c]]) for c in range(12))   # (PCM up to its count)
        assert np.array_equal(a[3][:12], b[3][:12])
        assert np.array_equal(a[4][:12], b[4][:12]) and np.array_equal(a[5][6:12], b[5][6:12])
        assert not np.array_equal(a[0][12:], b[0][12:])                 # (the followers themselves differ)
    assert any(len(set(res[0][0][5][c].tolist()) | set(res[0][1][5][c].tolist())) > 1 for c in range(6, 12))   # a scanner moved


def test_follow_toggled_between_calls_and_reset_keeps_the_flags(capi, P):
    M, bb, n = 8, 256, 10
    rng = np.random.default_rng(9)
    wide = rng.integers(96, 160, (1, 2 * 4 * bb * M), dtype=np.uint8)
    inc = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    shift = (np.arange(n) % 5 + 2).astype(np.uint8)
    h = capi.channelizer_default_taps(M)
    eng = capi.Engine(n, block_bytes=bb)
    eng.set_mode("fm")
    eng.set_rx_gain_db(7)
    z = capi.Channelizer(eng, M, n)
    z.set_channels(0, source=[0] * n, phase_inc=inc, gain_shift=shift)
    z.follow_gain(False)                              # accepted on channels that do not follow
    z.follow_gain(True, 3, 4)
    span = 4 * bb * M

    def check(piece, m0, following):
        got = _dev_call(eng, z, piece, bb)[0]
        for c in range(n):
            want = (gm.channel_db(wide[0], h, M, int(inc[c]), 7, P, m_range=(m0, m0 + 4 * bb // 2)) if c in following else
                    cm.channel(wide[0], h, M, int(inc[c]), int(shift[c]), P, m_range=(m0, m0 + 4 * bb // 2)))
            assert np.array_equal(got[c], want), (c, m0)

    check(wide[:, :span], 0, range(3, 7))
    z.follow_gain(False, 4, 2)                        # the set_channels shift is back in force
    check(wide[:, span:], 4 * bb // 2, (3, 6))
    z.reset()                                         # keeps the flags; the stream starts again from zero history
    check(wide[:, :span], 0, (3, 6))
    z.close()
    eng.close()


def test_every_refusal_and_nothing_queued_afterwards(capi, P, oracle, cases):
    case = cases["M8-7ch-lowpass"]
    eng = _engine(capi, case)
    z = _channelizer(capi, eng, case)
    calls = list(_pieces(case))

    def run(k, m_at):
        _set_manual(eng, case, k)
        rows, pcm, cnt, mag, alw = _dev_call(eng, z, calls[k][2], case.bb)
        _check_call(oracle, P, case, k, rows, pcm, cnt, mag, alw, eng.gain_trace(max(1, calls[k][1] // case.bb)), m_at)

    def refused(fn, *words):
        with pytest.raises(capi.IqdError) as err:
            fn()
        assert err.value.status == -1 and all(w in str(err.value) for w in words), str(err.value)

    run(0, 0)
    fol = int(np.nonzero(case.follow)[0][0])
    fixed = int(np.nonzero(~case.follow)[0][0])
    piece = calls[1][2]
    refused(lambda: z.run(piece), "follows its gain")
    d = eng.dev_alloc(piece.nbytes)
    refused(lambda: z.run_device(d, piece.shape[1], d), "follows its gain")
    z.set_survey(phase_inc=[0, 1 << 30])
    refused(lambda: z.survey(piece, case.bb), "survey", "follows its gain")
    refused(lambda: z.survey_device(d, piece.shape[1], case.bb, d), "survey", "follows its gain")
    eng.dev_free(d)
    refused(lambda: z.follow_scanner(True, fol, 1), "follows its gain", "scanner")
    refused(lambda: z.follow_scanner(True), "follows its gain", "scanner")       # a range with one such channel: nothing changes
    z.follow_scanner(True, fixed, 1)
    refused(lambda: z.follow_gain(True, fixed, 1), "follows its scanner", "gain")
    z.follow_scanner(False, fixed, 1)
    refused(lambda: z.follow_gain(True, len(case.src), 1), "range")
    for kw, words in ((dict(decimation_den=8), ("fractional", "gain")), (dict(sample_format="s8"), ("S8", "gain")),
                      (dict(sample_format="s16"), ("S16", "gain"))):
        zz = capi.Channelizer(eng, 75 if "decimation_den" in kw else 8, 2, **kw)
        refused(lambda: zz.follow_gain(True), *words)
        zz.follow_gain(False)
        zz.close()
    run(1, calls[0][1] // 2)                          # the stream stands where it stood
    run(2, (calls[0][1] + calls[1][1]) // 2)
    z.close()
    eng.close()


def test_the_loop_closes_on_the_operating_point(capi):
    """The weak and the medium carrier end within the AGC's deadband (1 dB) of its operating point (-12 dBFS); the same
    channels without follow_gain run to the rail, 46 dB."""
    M, bb, nblk = 8, 1024, 24
    wide = gc.capture(M, nblk * bb // 2 * M, 5)[None]
    for agc in (0, 1):
        for follow in (True, False):
            eng = capi.Engine(2, block_bytes=bb)
            eng.set_mode("fm")
            eng.agc_set_type(agc)
            eng.agc_enable(True)
            eng.set_gain_trace(True)
            z = capi.Channelizer(eng, M, 2)
            z.set_channels(0, source=[0, 0], phase_inc=[gc.inc_of(gc.CARRIERS[0][0]), gc.inc_of(gc.CARRIERS[1][0])])
            if follow:
                z.follow_gain(True)
            pcm, cnt, mag, alw = eng.accept_wideband(z, wide)
            gt = eng.gain_trace(nblk)
            for c in range(2):
                level = [capi.magnitude_dbfs(m) for m in mag[c, -4:]]
                if follow:
                    assert all(abs(v - (-12)) <= 1 for v in level), (agc, c, level, gt[c])
                    assert 0 < gt[c, -1] < 46 and len(set(gt[c, -4:].tolist())) == 1, (agc, c, gt[c])
                else:
                    assert gt[c, -1] == 46 and all(v < -13 for v in level), (agc, c, level, gt[c])
            z.close()
            eng.close()


def test_iqdemod_wide_agc_rxgain_and_gainlog_equal_the_python_path(capi, tmp_path):
    """iqdemod_wide agc= rxgain= gainlog=: its PCM and its log, byte for byte, against the device form with the same
    settings (calls of 2 blocks of 32768 bytes, then the capture's tail as one short block); the tool's refusals."""
    M, rate, blk = 8, 2048000, 32768 * 8
    wide = gc.capture(M, int(4.5 * blk) // 2, 61)
    wide = np.concatenate([wide, np.full(300, 128, np.uint8)])    # past the last 64 M: dropped
    n_bytes = len(wide) // (64 * M) * 64 * M
    cap = tmp_path / "cap.iq"
    wide.tofile(cap)
    offs = [300_000, -200_000, 700_000, 450_000]
    agc, rxgain, shifts = ["harris", "off", "lowpass"], [24, 30], [1, 2]
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_wide")
    base = [tool, "in=%s" % cap, "rate=%d" % rate, "offsets=" + ",".join(map(str, offs)), "modes=2", "blocks=2",
            "out=%s" % (tmp_path / "pcm_%d.s16")]
    r = subprocess.run(base + ["gains=1,2", "agc=" + ",".join(agc), "rxgain=24,30", "gainlog=%s" % (tmp_path / "gain.log")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    n = len(offs)
    eng = capi.Engine(n)
    eng.set_mode("fm")
    eng.set_gain_trace(True)
    z = capi.Channelizer(eng, M, n)
    z.set_channels(0, source=[0] * n, offset_hz=offs, fs=rate, gain_shift=[shifts[c % 2] for c in range(n)])
    for c in range(n):
        eng.set_rx_gain_db(rxgain[c % 2], c, 1)
        if agc[c % 3] != "off":
            eng.agc_set_type(1 if agc[c % 3] == "harris" else 0, c, 1)
            eng.agc_enable(True, c, 1)
    z.follow_gain(True)
    pcm, lines, at, b0 = [[] for _ in range(n)], [], 0, 0
    while at < n_bytes:
        part = wide[at:min(at + 2 * blk, n_bytes)]
        whole = len(part) // blk * blk
        for piece in (part[:whole], part[whole:]):
            if not len(piece):
                continue
            got = _dev_call(eng, z, piece.reshape(1, -1), 32768)
            nblk = got[4].shape[1]
            gt = eng.gain_trace(nblk)
            for c in range(n):
                pcm[c].append(got[1][c, :got[2][c]])
            lines += ["%d %d %d" % (b0 + b, c, min(int(gt[c, b]), 48)) for b in range(nblk) for c in range(n)]
            b0 += nblk
        at += len(part)
    assert (tmp_path / "gain.log").read_text().splitlines() == lines
    for c in range(n):
        assert np.array_equal(np.fromfile(tmp_path / ("pcm_%d.s16" % c), np.int16), np.concatenate(pcm[c])), c
    assert len({l.split()[2] for l in lines if l.split()[1] == "0"}) > 1   # channel 0's AGC moved its gain
    assert {l.split()[2] for l in lines if l.split()[1] == "1"} == {"30"}   # agc=off: the manual gain
    z.close()
    eng.close()
    for extra in (["agc=harris", "centre=100000000", "scan=99000000,101000000,100000"], ["rxgain=20", "decimation=75/8", "rate=2400000"],
                  ["agc=lowpass", "format=s8"], ["rxgain=20", "format=s16"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and len(r.stderr.strip().splitlines()) == 1 and "agc= / rxgain=" in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["agc=fast"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "agc must be" in r.stderr
