"""GPU (MI355X): scanner-driven wideband channels (include/iqdemod.h: iqd_channelizer_follow_scanner) bit for bit
against the model (tests/chan_scan_model.py: the oracle chain's scanner picks each block's increment), against the
host-driven one-block loop over today's API, beside fixed channels, across calls, through the device form, and at size."""
import os
import subprocess

import numpy as np
import pytest

from tests import chan_model as cm
from tests import chan_scan_model as sm

pytestmark = pytest.mark.gpu
BB = 4096                 # engine block_bytes: 2048 outputs per block
BO = BB // 2
BASE = 1_700_000_000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


def _capture(M, n_src, n_blocks, seed):
    """per source: four keyed carriers at fixed fractions of Fs, on in different blocks"""
    from rtlsdrdiags_amd import synth
    fs = 256000 * M
    spb = BO * M
    out = []
    for s in range(n_src):
        st = []
        for i, frac in enumerate((-0.3, -0.1, 0.15, 0.35)):
            on = [((i + s + k) % 5 * spb, ((i + s + k) % 5 + 2) * spb) for k in range(0, 3 * n_blocks, 5)]
            on = [(a + 5 * spb * j, b + 5 * spb * j) for j in range(n_blocks // 5 + 1) for a, b in on[:1]]
            st.append({"offset": int(frac * fs), "kind": ("fm", "am")[i % 2], "amplitude": 40.0, "on": on})
        out.append(synth.wideband(n_blocks * spb, fs, st, seed=seed + s, sigma=1.0))
    return np.stack(out)


def _centres(n_src):
    return [BASE + 3_000_000 * s for s in range(n_src)]


def _plan(M, n_ch, n_src, seed):
    """per channel: source, squelch threshold, scan grid (start, end, step) in station Hz"""
    rng = np.random.default_rng(seed)
    fs = 256000 * M
    src = (np.arange(n_ch) % n_src).astype(np.uint32)
    rng.shuffle(src)
    plans = []
    for c in range(n_ch):
        centre = _centres(n_src)[src[c]]
        step = int(0.05 * fs)
        kind = c % 4
        if kind == 0:      # a grid over the carriers: stops on them
            start = centre + int(-0.3 * fs) - 64000 - step * int(rng.integers(0, 3))
            end = start + step * 13
        elif kind == 1:    # runs out of the capture: silence, then wraps from the end to the start
            start = centre + int(0.15 * fs) - 64000
            end = start + step * 8
        elif kind == 2:    # never opens: scans and wraps
            start = centre + int(-0.1 * fs) - 64000
            end = start + step * 3
        else:              # always open: stays where start() put it
            start = centre + int(0.35 * fs) - 64000
            end = start + step * 2
        th = (-50, -50, 0, -200)[kind]
        plans.append((int(src[c]), th, (start, end, step)))
    return src, plans


def _engine(capi, n, plans, first=0, agc=None):
    eng = capi.Engine(first + n, block_bytes=BB)
    eng.set_mode("fm")
    for c, (_, th, grid) in enumerate(plans):
        eng.set_squelch(th, first + c, 1)
        eng.scanner_set_parameters(*grid, first=first + c, n=1)
        eng.scanner_start(True, first + c, 1)
    if agc is not None:
        eng.agc_set_type(agc)
        eng.agc_enable(True)
    eng.set_gain_trace(True)
    return eng


def _chains(plans, agc=None):
    from oracle.bindings import Oracle
    o = Oracle()
    out = []
    for _, th, grid in plans:
        c = o.chain()
        c.set_mode("fm")
        c.set_squelch(th)
        c.scanner_set_parameters(*grid)
        c.scanner_start()
        if agc is not None:
            c.agc_set_type(agc)
            c.agc_enable(True)
        out.append(c)
    return out


def _dev_call(eng, z, wide, first=0, bb=BB):
    """iqd_accept_wideband_device -> rows, pcm, counts, magnitude, allowed (bb: the engine's block_bytes)"""
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


@pytest.mark.parametrize("M,K,n_src,n_ch,calls", [
    (2, "default", 1, 7, [3, 2]), (3, "default", 3, 64, [4, 1]), (8, 1024, 1, 7, [2, 3]), (10, "default", 3, 300, [3]),
    (8, "default", 1, 1, [1, 4])])
def test_bit_identical_to_the_model(capi, P, M, K, n_src, n_ch, calls):
    rng = np.random.default_rng(M * 100 + n_ch)
    taps = None if K == "default" else rng.integers(-8000, 8001, K).astype(np.int16)
    h = capi.channelizer_default_taps(M) if taps is None else taps
    total = sum(calls)
    wide = _capture(M, n_src, total, seed=M + n_ch)
    src, plans = _plan(M, n_ch, n_src, seed=n_ch)
    eng = _engine(capi, n_ch, plans)
    z = capi.Channelizer(eng, M, n_ch, n_src, taps=taps)
    z.set_channels(0, source=src, phase_inc=[123456789] * n_ch, gain_shift=[c % 3 for c in range(n_ch)])
    z.set_source_frequency(_centres(n_src))
    z.follow_scanner(True)
    chans = _chains(plans)
    check = range(n_ch) if n_ch <= 64 else sorted(rng.choice(n_ch, 24, replace=False))
    at, traces = 0, []
    for k in calls:
        piece = wide[:, at * BO * M * 2:(at + k) * BO * M * 2]
        got = _dev_call(eng, z, piece)
        trace = eng.frequency_trace(k)
        traces.append(trace)
        for c in check:   # (the model's gain shift is per channel)
            s = plans[c][0]
            r, p, mg, a, tr = sm.follow(chans[c], wide[s], h, M, P, c % 3, _centres(n_src)[s], BO, k, m_first=at * BO)
            assert np.array_equal(got[0][c], r), (c, at)
            assert got[2][c] == len(p) and np.array_equal(got[1][c, :got[2][c]], p), c
            assert np.array_equal(got[3][c], mg) and np.array_equal(got[4][c], a), c
            assert np.array_equal(trace[c], tr), (c, trace[c], tr)
        at += k
    trace = np.concatenate(traces, 1)
    assert any(len(set(trace[c].tolist())) > 1 for c in range(n_ch))   # the scanners moved
    z.close()
    eng.close()


def _one_block_loop(capi, M, n_src, n_ch, src, plans, wide, nblk, shifts):
    """today's API: a plain channelizer run one block at a time, retuned from iqd_scanner_get + iqd_channelizer_tuning,
    out-of-band rows overwritten with 0x80, fed to iqd_accept_iq of a second engine"""
    eng = _engine(capi, n_ch, plans)
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=src, gain_shift=shifts)
    rows, pcm, mags, als, tr = [], [[] for _ in range(n_ch)], [], [], []
    for b in range(nblk):
        incs, silent = [], []
        for c in range(n_ch):
            f, _ = eng.scanner_tuned(c)
            d = capi.channelizer_tuning(M, _centres(n_src)[src[c]], f, 1)
            incs.append(0 if d is None else d)
            silent.append(d is None)
        z.set_channels(0, phase_inc=incs)
        r = z.run(wide[:, b * BO * M * 2:(b + 1) * BO * M * 2])
        r[np.array(silent)] = 0x80
        p, cnt, mg, al = eng.accept(r)
        for c in range(n_ch):
            pcm[c].append(p[c, :cnt[c]])
        rows.append(r)
        mags.append(mg)
        als.append(al)
        tr.append(eng.frequency_trace(1))
    z.close()
    eng.close()
    return (np.concatenate(rows, 1), [np.concatenate(x) for x in pcm], np.concatenate(mags, 1), np.concatenate(als, 1),
            np.concatenate(tr, 1))


def test_equals_the_host_driven_one_block_loop(capi):
    M, n_src, n_ch = 8, 2, 24
    wide = _capture(M, n_src, 20, seed=3)
    src, plans = _plan(M, n_ch, n_src, seed=4)
    shifts = [1] * n_ch
    ref = _one_block_loop(capi, M, n_src, n_ch, src, plans, wide, 20, shifts)
    eng = _engine(capi, n_ch, plans)
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=src, gain_shift=shifts)
    z.set_source_frequency(_centres(n_src))
    z.follow_scanner(True)
    rows, pcm, mags, als, tr = [], [[] for _ in range(n_ch)], [], [], []
    at = 0
    for k in (4, 16):
        got = _dev_call(eng, z, wide[:, at * BO * M * 2:(at + k) * BO * M * 2])
        rows.append(got[0])
        for c in range(n_ch):
            pcm[c].append(got[1][c, :got[2][c]])
        mags.append(got[3])
        als.append(got[4])
        tr.append(eng.frequency_trace(k))
        at += k
    assert np.array_equal(np.concatenate(rows, 1), ref[0])
    assert all(np.array_equal(np.concatenate(pcm[c]), ref[1][c]) for c in range(n_ch))
    assert np.array_equal(np.concatenate(mags, 1), ref[2]) and np.array_equal(np.concatenate(als, 1), ref[3])
    assert np.array_equal(np.concatenate(tr, 1), ref[4])
    assert ref[3].any() and not ref[3].all()
    z.close()
    eng.close()


@pytest.mark.parametrize("agc", [0, 1])
def test_agc_with_the_squelch(capi, P, agc):
    M, n_src, n_ch, nblk = 3, 1, 16, 6
    wide = _capture(M, n_src, nblk, seed=8)
    src, plans = _plan(M, n_ch, n_src, seed=9)
    plans = [(s, -60 + 3 * (c % 5), g) for c, (s, _, g) in enumerate(plans)]
    eng = _engine(capi, n_ch, plans, agc=agc)
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=src)
    z.set_source_frequency(_centres(n_src))
    z.follow_scanner(True)
    chans = _chains(plans, agc=agc)
    h = capi.channelizer_default_taps(M)
    got = _dev_call(eng, z, wide)
    trace, gtrace = eng.frequency_trace(nblk), eng.gain_trace(nblk)
    for c in range(n_ch):
        gains = []
        ch = chans[c]
        # the gain each block's squelch compared with: the model's chain before each block
        r, p, mg, a, tr = [], [], [], [], []
        for b in range(nblk):
            gains.append(ch.rx_gain_db())
            out = sm.follow(ch, wide[0], h, M, P, 0, _centres(1)[0], BO, 1, m_first=b * BO)
            r.append(out[0]); p.append(out[1]); a.append(out[3][0]); tr.append(out[4][0])
        assert np.array_equal(got[0][c], np.concatenate(r)), c
        assert np.array_equal(got[1][c, :got[2][c]], np.concatenate(p)), c
        assert np.array_equal(got[4][c], a) and np.array_equal(trace[c], tr), c
        assert np.array_equal(gtrace[c], gains), (c, gtrace[c], gains)
    assert any(len(set(gtrace[c].tolist())) > 1 for c in range(n_ch))   # the AGC moved the gain the squelch sees
    z.close()
    eng.close()


def test_following_beside_fixed_channels_and_across_calls(capi, P):
    M, n_src, n_ch = 8, 2, 40
    wide = _capture(M, n_src, 8, seed=12)
    src, plans = _plan(M, n_ch, n_src, seed=13)
    rng = np.random.default_rng(1)
    incs = rng.integers(0, 2 ** 32, n_ch).astype(np.uint64)
    follow = np.array([c % 3 != 0 for c in range(n_ch)])
    eng = _engine(capi, n_ch, plans)
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=src, phase_inc=incs)
    z.set_source_frequency(_centres(n_src))
    for c in np.nonzero(follow)[0]:
        z.follow_scanner(True, int(c), 1)
    fixed = np.nonzero(~follow)[0]
    e2 = capi.Engine(1)
    z2 = capi.Channelizer(e2, M, len(fixed), n_src)
    z2.set_channels(0, source=src[fixed], phase_inc=incs[fixed])
    chans = _chains(plans)
    h = capi.channelizer_default_taps(M)
    # calls: 2 blocks, one short block (half a block), 1 block after a reset of both, then follow off for channel 1
    sb = BO * M * 2
    pieces = [(0, 2 * sb), (2 * sb, 2 * sb + sb // 2)]
    m_at = 0
    for lo, hi in pieces:
        got = _dev_call(eng, z, wide[:, lo:hi])
        n_out = (hi - lo) // (2 * M)
        nblk = max(1, n_out // BO)
        bo = n_out // nblk
        assert np.array_equal(got[0][fixed], z2.run(wide[:, lo:hi]))
        tr = eng.frequency_trace(nblk)
        for c in np.nonzero(follow)[0][:10]:
            s = plans[c][0]
            r, p, mg, a, t = sm.follow(chans[c], wide[s], h, M, P, 0, _centres(n_src)[s], bo, nblk, m_first=m_at)
            assert np.array_equal(got[0][c], r) and np.array_equal(tr[c], t), c
            assert np.array_equal(got[1][c, :got[2][c]], p), c
        m_at += n_out
    # reset: the following flags and centres stay; the stream starts again from zero history
    z.reset()
    z2.reset()
    z.follow_scanner(False, 1, 1)
    got = _dev_call(eng, z, wide[:, :sb])
    assert np.array_equal(got[0][fixed], z2.run(wide[:, :sb]))
    assert np.array_equal(got[0][1], cm.channel(wide[src[1]], h, M, int(incs[1]), 0, P, m_range=(0, BO)))
    z.follow_scanner(True, 1, 1)
    assert np.array_equal(_dev_call(eng, z, wide[:, sb:2 * sb])[0][fixed], z2.run(wide[:, sb:2 * sb]))
    z.close(); z2.close()
    eng.close(); e2.close()


def test_rotation_scanner_commands_and_engine_reset_between_calls(capi, P):
    """Settings changed between calls reach the walker once, before it reads state: rotation selectors 0 and -1, scanners
    stopped, given new parameters and started (the jump to the new end frequency), restarted without new parameters,
    and a reset of the engine's demodulators."""
    M, n_src, n_ch, k = 8, 1, 12, 2
    wide = _capture(M, n_src, 5 * k, seed=41)
    src, plans = _plan(M, n_ch, n_src, seed=42)
    centre, fs = _centres(1)[0], 256000 * M
    eng = _engine(capi, n_ch, plans)
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=src)
    z.set_source_frequency([centre])
    z.follow_scanner(True)
    chans = _chains(plans)
    h = capi.channelizer_default_taps(M)
    rot = [1] * n_ch
    traces = []

    def call(at):
        got = _dev_call(eng, z, wide[:, at * BO * M * 2:(at + k) * BO * M * 2])
        tr = eng.frequency_trace(k)
        for c in range(n_ch):
            r, p, mg, a, t = sm.follow(chans[c], wide[0], h, M, P, 0, centre, BO, k, m_first=at * BO, rotation=rot[c])
            assert np.array_equal(got[0][c], r), (c, at)
            assert got[2][c] == len(p) and np.array_equal(got[1][c, :got[2][c]], p), (c, at)
            assert np.array_equal(got[3][c], mg) and np.array_equal(got[4][c], a), (c, at)
            assert np.array_equal(tr[c], t), (c, at, tr[c], t)
        traces.append(tr)

    call(0)
    for c in range(8):                               # rotation: 0 for channels 0-3, -1 for 4-7
        rot[c] = 0 if c < 4 else -1
        eng.set_rotation(rot[c], c, 1)
        chans[c].set_rotation(rot[c])
    call(k)
    for c in (8, 9):                                 # stopped: the channel stays where the scan stopped
        eng.scanner_start(False, c, 1)
        chans[c].scanner_stop()
    grid = (centre - int(0.2 * fs) - 64000, centre + int(0.1 * fs) - 64000, int(0.05 * fs))
    for c in (10, 11):                               # stop, new parameters, start: a jump to the new end frequency
        eng.scanner_start(False, c, 1)
        chans[c].scanner_stop()
        eng.scanner_set_parameters(*grid, first=c, n=1)
        chans[c].scanner_set_parameters(*grid)
        eng.scanner_start(True, c, 1)
        chans[c].scanner_start()
    call(2 * k)
    assert all(len(set(traces[-1][c].tolist())) == 1 for c in (8, 9))
    assert traces[-1][10][0] in (grid[1], grid[0])   # the first block was cut at the new end frequency
    eng.reset()                                      # the demodulators' state, between calls
    for ch in chans:
        ch.reset()
    for c in (8, 9):                                 # restarted without new parameters: no jump
        eng.scanner_start(True, c, 1)
        chans[c].scanner_start()
    call(3 * k)
    call(4 * k)
    z.close()
    eng.close()


def _tool_capture(M, n_blocks, seed):
    """keyed carriers for the tool: engine blocks of 32768 bytes"""
    from rtlsdrdiags_amd import synth
    fs, spb = 256000 * M, 16384 * M
    stations = [{"offset": -600_000, "kind": "fm", "amplitude": 40.0, "on": [(2 * spb, 5 * spb)]},
                {"offset": 300_000, "kind": "am", "amplitude": 40.0, "on": [(0, 2 * spb), (6 * spb, 9 * spb)]},
                {"offset": 100_000, "kind": "fm", "amplitude": 40.0, "on": [(4 * spb, 8 * spb)]}]
    return synth.wideband(int(n_blocks * spb), fs, stations, seed=seed, sigma=1.0)


def test_iqdemod_wide_scan_and_freqlog_equal_the_python_path(capi, tmp_path):
    """iqdemod_wide centre= scan= squelch= freqlog=: its PCM and its log, byte for byte, against the device form with the
    same settings (calls of 4 blocks, then the capture's tail as one short block)."""
    M, rate, n_bytes = 8, 2048000, int(9.5 * 32768 * 8)
    centre = BASE
    wide = _tool_capture(M, 9.5, seed=51)
    wide = np.concatenate([wide, np.full(300, 128, np.uint8)])    # past the last 64 M: dropped
    cap = tmp_path / "cap.iq"
    wide.tofile(cap)
    offs = [100_000, -200_000, 364_000, 0]
    grids = [(centre - 664_000, centre + 336_000, 100_000), (centre + 700_000, centre + 1_200_000, 250_000), (0, 0, 0)]
    squelch = [-50, -40]
    tool = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_wide")
    r = subprocess.run([tool, "in=%s" % cap, "decimation=8", "rate=2048000", "offsets=" + ",".join(map(str, offs)),
                        "modes=2,1", "centre=%d" % centre, "scan=" + ",".join("%d" % v for g in grids for v in g),
                        "squelch=" + ",".join(map(str, squelch)), "freqlog=%s" % (tmp_path / "freq.log"),
                        "out=%s" % (tmp_path / "pcm_%d.s16")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    n = len(offs)
    eng = capi.Engine(n)
    z = capi.Channelizer(eng, M, n)
    z.set_channels(0, source=[0] * n, offset_hz=offs, fs=rate)
    z.set_source_frequency([centre])
    eng.set_gain_trace(True)
    cut, follows = [], []
    for c in range(n):
        eng.set_mode(("fm", "am")[c % 2], c, 1)
        eng.set_squelch(squelch[c % 2], c, 1)
        g = grids[c % 3]
        follows.append(any(g))
        if any(g):
            eng.scanner_set_parameters(*g, first=c, n=1)
            eng.scanner_start(True, c, 1)
            z.follow_scanner(True, c, 1)
            cut.append(g[1])                          # start() after new parameters: the end frequency
        else:
            cut.append(centre + offs[c] - 64000)
    pcm = [[] for _ in range(n)]
    lines, blk = [], 0
    call, block = 4 * 32768 * M, 32768 * M
    for a in range(0, n_bytes, call):
        part = wide[a:min(a + call, n_bytes)]
        whole = len(part) // block * block
        for piece in (part[:whole], part[whole:]):
            if not len(piece):
                continue
            got = _dev_call(eng, z, piece.reshape(1, -1), bb=32768)
            nblk = got[4].shape[1]
            tr = eng.frequency_trace(nblk)
            for c in range(n):
                pcm[c].append(got[1][c, :got[2][c]])
            for b in range(nblk):
                for c in range(n):
                    lines.append("%d %d %d %d" % (blk + b, c, cut[c], got[4][c, b]))
                    if follows[c]:
                        cut[c] = int(tr[c, b])
            blk += nblk
    assert (tmp_path / "freq.log").read_text().splitlines() == lines
    for c in range(n):
        assert np.array_equal(np.fromfile(tmp_path / ("pcm_%d.s16" % c), np.int16), np.concatenate(pcm[c])), c
    opened = [int(l.split()[3]) for l in lines]
    assert 0 < sum(opened) < len(opened)
    assert len({l.split()[2] for l in lines if l.split()[1] == "0"}) > 2   # channel 0 scanned
    z.close()
    eng.close()


def test_device_form_equals_host_form_and_argument_errors(capi):
    M, n_src, n_ch = 8, 1, 16
    wide = _capture(M, n_src, 3, seed=21)
    src, plans = _plan(M, n_ch, n_src, seed=22)
    res = []
    for dev in (False, True):
        eng = _engine(capi, n_ch, plans)
        z = capi.Channelizer(eng, M, n_ch, n_src)
        z.set_channels(0, source=src)
        z.set_source_frequency(_centres(n_src))
        z.follow_scanner(True)
        if dev:
            res.append(_dev_call(eng, z, wide)[1:])
        else:
            res.append(eng.accept_wideband(z, wide))
        res[-1] = res[-1] + (eng.frequency_trace(3),)
        if dev:
            with pytest.raises(capi.IqdError):
                z.run(wide)
            d = eng.dev_alloc(wide.nbytes + 64)
            with pytest.raises(capi.IqdError):
                z.run_device(d, wide.shape[1], d)
            with pytest.raises(capi.IqdError):   # misaligned rows
                eng.accept_wideband_device(z, d, wide.shape[1], d + 8, d)
            with pytest.raises(capi.IqdError):
                z.follow_scanner(True, n_ch, 1)
            with pytest.raises(capi.IqdError):
                z.set_source_frequency([0, 0])
            with pytest.raises(capi.IqdError):
                eng.accept_wideband_device(z, d, wide.shape[1], d, d, first=1)
            eng.dev_free(d)
        z.close()
        eng.close()
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)


def test_at_size_4096_channels_16_sources(capi, P):
    M, n_src, n_ch = 8, 16, 4096
    n_out = 2 ** 16
    nblk = n_out // BO
    wide = _capture(M, n_src, nblk, seed=31)
    src, plans = _plan(M, n_ch, n_src, seed=32)
    eng = _engine(capi, n_ch, plans)
    z = capi.Channelizer(eng, M, n_ch, n_src)
    z.set_channels(0, source=src)
    z.set_source_frequency(_centres(n_src))
    z.follow_scanner(True)
    got = _dev_call(eng, z, wide)
    tr = eng.frequency_trace(nblk)
    al = got[4]
    for c in range(n_ch):   # the trace agrees with signal_present: one step or the wrap per rejected block, else no move
        start, end, step = plans[c][2]
        prev = end
        for b in range(nblk):
            if al[c, b]:
                assert tr[c, b] == prev, (c, b)
            else:
                want = prev + step if prev + step <= end else start
                assert tr[c, b] == want, (c, b)
            prev = int(tr[c, b])
    rng = np.random.default_rng(33)
    chans = {}
    h = capi.channelizer_default_taps(M)
    sample = sorted(rng.choice(n_ch, 64, replace=False))
    pl = [plans[c] for c in sample]
    for c, ch in zip(sample, _chains(pl)):
        s = plans[c][0]
        r, p, mg, a, t = sm.follow(ch, wide[s], h, M, P, 0, _centres(n_src)[s], BO, nblk)
        assert np.array_equal(got[0][c], r) and np.array_equal(tr[c], t), c
        assert np.array_equal(got[1][c, :got[2][c]], p) and np.array_equal(got[3][c], mg), c
    z.close()
    eng.close()
