"""GPU (MI355X): track-following wideband channels (include/iqdemod.h: "Track-following channels") bit for bit against the
model (tests/chan_track_model.py) on the inputs of tests/chan_track_cases.py in every call form, against a block-by-block
host loop through fixed channels and chz_kernel (an oracle that does not rest on the model), across call splits, beside
fixed, scanner- and gain-following channels, through every refusal, and queued behind spectrum, detector and tracker on one
stream.  Every comparison is exact equality."""
import numpy as np
import pytest

from tests import chan_gain_cases as gc
from tests import chan_model as cm
from tests import chan_track_cases as tc
from tests import chan_track_model as tm

pytestmark = pytest.mark.gpu
THRESHOLD = -45


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def cases(capi, P):
    return {c.name: c for c in tc.cases(capi, P)}


_TRUTH = {}


def truth(oracle, P, case):
    """The model's run of a case, computed once: per run of the script [n_ch] rows, and what the oracle chain of every
    channel makes of them (pcm, magnitude, allowed), each a list per run."""
    if case.name not in _TRUTH:
        n = len(case.src)
        rows = [tc.run_model(tm, cm, case, P, c) for c in range(n)]
        runs = len(rows[0])
        acc = []
        for c in range(n):
            ch = oracle.chain()
            ch.set_mode("fm")
            ch.set_squelch(THRESHOLD)
            acc.append([ch.accept_stream(rows[c][k], block_bytes=tc.ENGINE_BB) for k in range(runs)])
            ch.close()
        _TRUTH[case.name] = ([np.stack([rows[c][k] for c in range(n)]) for k in range(runs)], acc)
    return _TRUTH[case.name]


def _engine(capi, n):
    eng = capi.Engine(n, block_bytes=tc.ENGINE_BB)
    eng.set_mode("fm")
    eng.set_squelch(THRESHOLD)
    return eng


def _channelizer(capi, eng, case):
    z = capi.Channelizer(eng, case.M, len(case.src), case.n_src, taps=case.taps)
    z.set_channels(0, source=case.src, phase_inc=case.inc, gain_shift=case.shift)
    z.follow_tracks(case.slot)
    return z


def _upload(eng, a):
    a = np.ascontiguousarray(a)
    d = eng.dev_alloc(max(a.nbytes, 16))
    eng.dev_upload(d, a.view(np.uint8).reshape(-1))
    return d


def _dev_accept(eng, z, wide, first=0):
    """iqd_accept_wideband_device -> rows, pcm, counts, magnitude, allowed"""
    n, bps = z.n_channels, wide.shape[1]
    row = bps // z.decimation
    nblk = row // tc.ENGINE_BB
    d_w, d_r = _upload(eng, wide), eng.dev_alloc(n * row)
    d_p, d_c = eng.dev_alloc(n * row // 64 * 2), eng.dev_alloc(4 * n)
    d_m, d_a = eng.dev_alloc(4 * n * nblk), eng.dev_alloc(n * nblk)
    try:
        eng.accept_wideband_device(z, d_w, bps, d_r, d_p, d_c, d_m, d_a, first=first)
        eng.synchronize()
        return (eng.dev_download(d_r, n * row).reshape(n, row),
                eng.dev_download(d_p, n * row // 64 * 2, np.int16).reshape(n, -1),
                eng.dev_download(d_c, 4 * n, np.uint32), eng.dev_download(d_m, 4 * n * nblk, np.uint32).reshape(n, nblk),
                eng.dev_download(d_a, n * nblk).reshape(n, nblk))
    finally:
        for d in (d_w, d_r, d_p, d_c, d_m, d_a):
            eng.dev_free(d)


def _dev_run(eng, z, wide):
    n, bps = z.n_channels, wide.shape[1]
    row = bps // z.decimation
    d_w, d_r = _upload(eng, wide), eng.dev_alloc(n * row)
    try:
        z.run_device(d_w, bps, d_r)
        eng.synchronize()
        return eng.dev_download(d_r, n * row).reshape(n, row)
    finally:
        eng.dev_free(d_w)
        eng.dev_free(d_r)


def _set_table(eng, z, case, t, keep):
    d = _upload(eng, case.table[:, t * case.nblk:(t + 1) * case.nblk])
    keep.append(d)
    z.set_track_table(d, case.S, case.nblk, case.bb, case.lag, case.min_state)


def _script(capi, oracle, P, case, form, between=None):
    """The case's script in one call form, every run against the truth.  between(k, eng, z): called before run k."""
    want_rows, want_acc = truth(oracle, P, case)
    n = len(case.src)
    eng = _engine(capi, n)
    z = _channelizer(capi, eng, case)
    span, pos, k, keep = case.nblk * case.bb * case.M, 0, 0, []
    for op in case.script:
        if op[0] == "reset":
            z.reset()
            pos = 0
        elif op[0] in ("stop", "start"):
            for c in (tc.some(case) if op[1] == "some" else op[1]):
                z.follow_tracks([int(case.slot[c]) if op[0] == "start" else -1], first=c)
        else:
            if between:
                between(k, eng, z)
            _set_table(eng, z, case, op[1], keep)
            piece = case.wide[:, pos * span:(pos + 1) * span]
            rows = acc = None
            if form == "run":
                rows = z.run(piece)
            elif form == "run_device":
                rows = _dev_run(eng, z, piece)
            elif form == "accept":
                acc = eng.accept_wideband(z, piece)
            else:
                got = _dev_accept(eng, z, piece)
                rows, acc = got[0], got[1:]
            if rows is not None:
                bad = [c for c in range(n) if not np.array_equal(rows[c], want_rows[k][c])]
                assert not bad, (case.name, form, k, bad)
            if acc is not None:
                pcm, cnt, mag, alw = acc
                for c in range(n):
                    p, mg, al = want_acc[c][k]
                    assert cnt[c] == len(p) and np.array_equal(pcm[c, :cnt[c]], p), (case.name, form, k, c)
                    assert np.array_equal(mag[c], mg) and np.array_equal(alw[c], al), (case.name, form, k, c)
            pos += 1
            k += 1
    z.close()
    for d in keep:
        eng.dev_free(d)
    eng.close()


@pytest.mark.parametrize("form", ["run", "run_device", "accept", "accept_device"])
@pytest.mark.parametrize("name", tc.case_names())
def test_bit_identical_to_the_model(capi, P, oracle, cases, name, form):
    """rows through the run forms; rows, PCM, magnitudes and flags through the accept forms; host and device pointers.
    The script case also stops and starts followers (the set_channels increment is back in force) and resets."""
    _script(capi, oracle, P, cases[name], form)


def _synthetic(rng, n_src, n_blocks, S):
    t = tc.synthetic_table(rng, n_src, n_blocks, S, n_blocks)
    return t


@pytest.mark.parametrize("n_ch,n_src,S,min_state,K", [(20, 1, 8, 2, None), (4096, 16, 64, 1, None), (4096, 16, 64, 2, 1000)])
def test_equal_to_a_host_loop_of_one_block_calls_through_fixed_channels(capi, n_ch, n_src, S, min_state, K):
    """An oracle that does not rest on the model: per block the slots are downloaded, set_channels gets their phase_inc,
    chz_kernel cuts one block, and 0x80 goes over the rows that are not live.  4096 followers: workgroup rows of 8 tiles;
    with K = 1000 taps the operands of one table block are 32 MiB, so the call is cut into two runs of two blocks."""
    M, bb, nblk = 8, 256, 4
    rng = np.random.default_rng(n_ch)
    taps = None if K is None else rng.integers(-30, 31, K).astype(np.int16)
    wide = rng.integers(0, 256, (n_src, nblk * bb * M), dtype=np.uint8)
    src = (np.arange(n_ch) % n_src).astype(np.uint32)
    slot = ((np.arange(n_ch) // n_src * 5 + 3) % S).astype(np.int32)
    L = (np.arange(n_ch) % 9).astype(np.uint8)
    table = _synthetic(rng, n_src, nblk, S)
    eng = _engine(capi, 1)
    z = capi.Channelizer(eng, M, n_ch, n_src, taps=taps)
    z.set_channels(0, source=src, phase_inc=rng.integers(0, 2 ** 32, n_ch, dtype=np.uint64), gain_shift=L)   # (the increments: ignored)
    z.follow_tracks(slot)
    d_t = _upload(eng, table)
    z.set_track_table(d_t, S, nblk, bb, 0, min_state)
    got = _dev_run(eng, z, wide)
    z2 = capi.Channelizer(eng, M, n_ch, n_src, taps=taps)
    z2.set_channels(0, source=src, gain_shift=L)
    want = np.empty_like(got)
    for b in range(nblk):
        slots = eng.dev_download(d_t, table.nbytes).view(capi.TRACK_SLOT).reshape(n_src, nblk, S)[:, b]
        mine = slots[src, slot]
        z2.set_channels(0, phase_inc=mine["phase_inc"])
        rows = z2.run(wide[:, b * bb * M:(b + 1) * bb * M])
        rows[mine["state"] < min_state] = 0x80
        want[:, b * bb:(b + 1) * bb] = rows
    assert np.array_equal(got, want)
    live = table["state"][src[:, None], np.arange(nblk)[None, :], slot[:, None]] >= min_state
    assert live.any() and not live.all() and len(set(got[live[:, 0]][:, :bb].tobytes())) > 2
    z.close()
    z2.close()
    eng.dev_free(d_t)
    eng.close()


def test_one_call_of_twelve_blocks_twelve_calls_of_one_and_five_plus_seven(capi, cases):
    case = cases["M2-9f-S8-b256"]
    assert case.lag == 1 and case.nblk == 12
    res = []
    for cuts in ([12], [1] * 12, [5, 7]):
        eng = _engine(capi, len(case.src))
        z = _channelizer(capi, eng, case)
        rows, b, keep = [], 0, []
        for n in cuts:
            d = _upload(eng, case.table[:, b:b + n])
            keep.append(d)
            z.set_track_table(d, case.S, n, case.bb, 1, case.min_state)
            rows.append(_dev_run(eng, z, case.wide[:, b * case.bb * case.M:(b + n) * case.bb * case.M]))
            b += n
        res.append(np.concatenate(rows, 1))
        z.close()
        for d in keep:
            eng.dev_free(d)
        eng.close()
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[2])


def test_fixed_scanner_and_gain_following_channels_are_what_they_are_without_track_followers(capi):
    M, bb, nblk, n = 8, 1024, 6, 28
    fs, base = 256000 * M, 1_700_000_000
    wide = gc.capture(M, nblk * bb // 2 * M, 77, sigma=1.0)[None]
    rng = np.random.default_rng(5)
    inc = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    inc[12:20] = [gc.inc_of(gc.CARRIERS[c % 3][0]) for c in range(8)]
    table = np.zeros((1, 6, 8), capi.TRACK_SLOT)      # 6 table blocks of 512 row bytes per call: not the engine's blocks
    table["state"], table["track_id"] = 2, 1
    table["phase_inc"] = rng.integers(0, 2 ** 32, table.shape, dtype=np.uint64)
    res = []
    for with_tracks in (True, False):
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
        z.follow_gain(True, 12, 8)
        d_t = _upload(eng, table)
        if with_tracks:
            z.follow_tracks(np.arange(8), first=20)
            z.set_track_table(d_t, 8, 6, 512, 0, 2)
        out = []
        for half in range(2):
            piece = wide[:, half * nblk * bb * M // 2:(half + 1) * nblk * bb * M // 2]
            n_, bps = n, piece.shape[1]
            row = bps // M
            nb = row // bb
            d_w, d_r = _upload(eng, piece), eng.dev_alloc(n_ * row)
            d_p, d_c, d_m, d_a = eng.dev_alloc(n_ * row // 64 * 2), eng.dev_alloc(4 * n_), eng.dev_alloc(4 * n_ * nb), eng.dev_alloc(n_ * nb)
            eng.accept_wideband_device(z, d_w, bps, d_r, d_p, d_c, d_m, d_a)
            eng.synchronize()
            out.append((eng.dev_download(d_r, n_ * row).reshape(n_, row), eng.dev_download(d_p, n_ * row // 64 * 2, np.int16).reshape(n_, -1),
                        eng.dev_download(d_c, 4 * n_, np.uint32), eng.dev_download(d_m, 4 * n_ * nb, np.uint32).reshape(n_, nb),
                        eng.dev_download(d_a, n_ * nb).reshape(n_, nb), eng.frequency_trace(nb), eng.gain_trace(nb)))
            for d in (d_w, d_r, d_p, d_c, d_m, d_a):
                eng.dev_free(d)
        res.append(out)
        z.close()
        eng.dev_free(d_t)
        eng.close()
    for a, b in zip(*res):
        assert np.array_equal(a[0][:20], b[0][:20]) and np.array_equal(a[2][:20], b[2][:20])
        assert all(np.array_equal(a[1][c, :a[2][c]], b[1][c, :b[2][c]]) for c in range(20))   # (PCM up to its count)
        assert np.array_equal(a[3][:20], b[3][:20]) and np.array_equal(a[4][:20], b[4][:20])
        assert np.array_equal(a[5][6:12], b[5][6:12]) and np.array_equal(a[6][12:20], b[6][12:20])
        assert not np.array_equal(a[0][20:], b[0][20:])                 # (the followers themselves differ)


def test_every_refusal_and_nothing_queued_afterwards(capi, P, oracle, cases):
    case = cases["M2-9f-S8-b256"]
    fol = int(np.nonzero(case.slot >= 0)[0][0])
    fixed = int(np.nonzero(case.slot < 0)[0][0])
    n = len(case.src)

    def refused(fn, *words):
        with pytest.raises(capi.IqdError) as err:
            fn()
        assert err.value.status == -1 and all(w in str(err.value) for w in words), str(err.value)

    def between(k, eng, z):
        if k != 1:
            return
        piece = case.wide[:, :case.nblk * case.bb * case.M]
        d = eng.dev_alloc(4096)
        good = dict(n_slots=case.S, n_blocks=case.nblk, block_bytes=case.bb, lag=case.lag, min_state=case.min_state)
        for bad, word in ((dict(reserved=(0, 1, 0)), "reserved"), (dict(n_slots=0), "n_slots"), (dict(n_slots=65), "n_slots"),
                          (dict(n_blocks=0), "n_blocks"), (dict(block_bytes=0), "block_bytes"), (dict(block_bytes=96), "block_bytes"),
                          (dict(lag=2), "lag"), (dict(min_state=0), "min_state"), (dict(min_state=3), "min_state")):
            refused(lambda: z.set_track_table(d, **dict(good, **bad)), word)
        refused(lambda: z.set_track_table(0, **good), "slots_dev", "NULL")
        refused(lambda: z.set_track_table(d + 8, **good), "slots_dev", "aligned")
        refused(lambda: z.follow_tracks([-2], first=fol), "slot")
        refused(lambda: z.follow_tracks([64], first=fol), "slot")
        refused(lambda: z.follow_tracks([0], first=n), "range")
        refused(lambda: z.follow_tracks([0, 0], first=n - 1), "range")
        refused(lambda: z.follow_scanner(True, fol, 1), "track slot")
        refused(lambda: z.follow_gain(True, fol, 1), "track slot")
        refused(lambda: z.follow_gain(True), "track slot")                # a range with such a channel: nothing changes
        z.follow_scanner(True, fixed, 1)
        refused(lambda: z.follow_tracks([0], first=fixed), "follows its scanner")
        z.follow_scanner(False, fixed, 1)
        z.follow_gain(True, fixed, 1)
        refused(lambda: z.follow_tracks([0], first=fixed), "follows its gain")
        z.follow_gain(False, fixed, 1)
        for kw, words in ((dict(decimation_den=8), ("fractional",)), (dict(sample_format="s8"), ("S8",)),
                          (dict(sample_format="s16"), ("S16",))):
            zz = capi.Channelizer(eng, 75 if "decimation_den" in kw else 8, 2, **kw)
            refused(lambda: zz.follow_tracks([0, 1]), "tracks", *words)
            zz.follow_tracks(None)
            zz.follow_tracks([-1, -1])
            zz.close()
        # at a call: no table, a slot the table does not have, the length rule - in every call form
        calls = (lambda: z.run(piece), lambda: z.run_device(d, piece.shape[1], d), lambda: eng.accept_wideband(z, piece),
                 lambda: eng.accept_wideband_device(z, d, piece.shape[1], d, d))
        z.set_track_table(None)
        for call in calls:
            refused(call, "no track table")
        z.set_track_table(d, **dict(good, n_slots=1))
        for call in calls:
            refused(call, "n_slots")
        z.set_track_table(d, **dict(good, n_blocks=case.nblk - 1))
        for call in calls:
            refused(call, "n_blocks * block_bytes")
        z.set_survey(phase_inc=[0, 1 << 30])
        refused(lambda: z.survey(piece, case.bb), "survey", "track slot")
        refused(lambda: z.survey_device(d, piece.shape[1], case.bb, d), "survey", "track slot")
        eng.dev_free(d)

    _script(capi, oracle, P, case, "accept_device", between=between)      # the stream stands where it stood: runs 1 and 2 are right


def test_spectrum_detector_tracker_and_channelizer_on_one_stream_with_one_synchronise(capi, P, oracle, cases):
    """capture -> spectrum -> detector -> tracker -> accept_wideband_device, three calls of 8 blocks queued back to back and
    one synchronise at the end: the rows, PCM, magnitudes and flags of the models' chain (the chained case)."""
    from tests import track_cases as trc
    case = cases["M8-chained"]
    want_rows, want_acc = truth(oracle, P, case)
    k = trc.CHAINED
    N, F, nb, K, S, M = k["N"], k["F"], k["blocks"], 16, k["S"], case.M
    n, per = len(case.src), case.nblk
    eng = _engine(capi, n)
    s, d = capi.Spectrum(eng, N), capi.Detector(eng, N)
    t = capi.Tracker(eng, N, n_slots=S, gate_q8=k["G"], open_hits=k["H"], hold_blocks=k["B"], alpha_q8=k["A"])
    z = _channelizer(capi, eng, case)
    wide_bytes = 2 * N * F                          # one table block of the capture
    row = per * case.bb
    d_in = _upload(eng, case.wide)
    d_pow, d_rows, d_det = eng.dev_alloc(4 * N * nb), eng.dev_alloc(16 * nb), eng.dev_alloc(32 * nb * K)
    d_slots, d_blocks = eng.dev_alloc(32 * nb * S), eng.dev_alloc(16 * nb)
    outs = []
    for c in range(3):
        b0 = c * per
        o = (eng.dev_alloc(n * row), eng.dev_alloc(n * row // 64 * 2), eng.dev_alloc(4 * n), eng.dev_alloc(4 * n * (row // tc.ENGINE_BB)),
             eng.dev_alloc(n * (row // tc.ENGINE_BB)))
        outs.append(o)
        s.run_device(d_in + b0 * wide_bytes, per * wide_bytes, F, d_pow + b0 * N * 4)
        d.run_device(d_pow + b0 * N * 4, per, d_rows + 16 * b0, d_det + 32 * K * b0)
        t.run_device(d_rows + 16 * b0, d_det + 32 * K * b0, per, d_slots + 32 * S * b0, d_blocks + 16 * b0)
        z.set_track_table(d_slots + 32 * S * b0, S, per, case.bb, case.lag, case.min_state)
        eng.accept_wideband_device(z, d_in + b0 * wide_bytes, per * wide_bytes, *o)
    eng.synchronize()
    slots = eng.dev_download(d_slots, 32 * nb * S).view(capi.TRACK_SLOT).reshape(1, nb, S)
    assert np.array_equal(slots, case.table)
    nblk = row // tc.ENGINE_BB
    for c, o in enumerate(outs):
        rows = eng.dev_download(o[0], n * row).reshape(n, row)
        pcm = eng.dev_download(o[1], n * row // 64 * 2, np.int16).reshape(n, -1)
        cnt = eng.dev_download(o[2], 4 * n, np.uint32)
        mag = eng.dev_download(o[3], 4 * n * nblk, np.uint32).reshape(n, nblk)
        alw = eng.dev_download(o[4], n * nblk).reshape(n, nblk)
        assert np.array_equal(rows, want_rows[c]), c
        for ch in range(n):
            p, mg, al = want_acc[ch][c]
            assert cnt[ch] == len(p) and np.array_equal(pcm[ch, :cnt[ch]], p), (c, ch)
            assert np.array_equal(mag[ch], mg) and np.array_equal(alw[ch], al), (c, ch)
    assert any((r != 0x80).any() for r in want_rows) and any((r == 0x80).all(axis=1).any() for r in want_rows)
    for o in outs:
        for p in o:
            eng.dev_free(p)
    for p in (d_in, d_pow, d_rows, d_det, d_slots, d_blocks):
        eng.dev_free(p)
    for obj in (z, t, d, s):
        obj.close()
    eng.close()


def test_iqdemod_wide_tracks_and_tracklog_equal_the_python_path(capi, tmp_path):
    """iqdemod_wide tracks= tracklog=: its PCM and its log, byte for byte, against the device chain queued from Python with
    the same settings - calls of 8 table blocks, a last call of the 4 whole blocks left, the trailing bytes dropped; the
    tool's refusals."""
    import math
    import os
    import subprocess
    from tests import track_cases as trc
    k = trc.CHAINED
    N, F, S, M, rate, per = k["N"], k["F"], k["S"], trc.RATE // 256000, trc.RATE, 8
    wide_block = 2 * N * F
    bb = wide_block // M
    whole = trc.chained_wide().reshape(-1)
    wide = np.concatenate([whole[:20 * wide_block], np.full(300, 128, np.uint8)])   # 20 table blocks and a part of one
    cap = tmp_path / "cap.iq"
    wide.tofile(cap)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "rtlsdrdiags_amd", "bin", "iqdemod_wide")
    modes, gains, lag = [2, 1], [2, 3], 1
    base = [tool, "in=%s" % cap, "rate=%d" % rate, "modes=2,1", "out=%s" % (tmp_path / "pcm_%d.s16")]
    args = base + ["tracks=%d" % S, "bins=%d" % N, "frames=%d" % F, "gains=2,3", "blocks=%d" % per, "lag=%d" % lag,
                   "tracklog=%s" % (tmp_path / "track.log")]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "300 trailing bytes" in r.stderr
    eng = capi.Engine(S, block_bytes=bb)
    for c in range(S):
        eng.set_mode({1: "am", 2: "fm"}[modes[c % 2]], c, 1)
    eng.set_rotation(0)
    s, d = capi.Spectrum(eng, N), capi.Detector(eng, N)
    t = capi.Tracker(eng, N, n_slots=S)
    z = capi.Channelizer(eng, M, S)
    z.set_channels(0, source=[0] * S, phase_inc=[0] * S, gain_shift=[gains[c % 2] for c in range(S)])
    z.follow_tracks(np.arange(S))
    K = 16
    d_in, d_pow = eng.dev_alloc(per * wide_block), eng.dev_alloc(4 * N * per)
    d_rows, d_det, d_slots, d_blocks = eng.dev_alloc(16 * per), eng.dev_alloc(32 * per * K), eng.dev_alloc(32 * per * S), eng.dev_alloc(16 * per)
    d_out, d_pcm, d_cnt = eng.dev_alloc(S * per * bb), eng.dev_alloc(S * per * bb // 64 * 2), eng.dev_alloc(4 * S)
    pcm, lines, carry, b_no = [[] for _ in range(S)], [], [(0, 0)] * S, 0
    for b0 in range(0, 20, per):
        nb = min(per, 20 - b0)
        eng.dev_upload(d_in, wide[b0 * wide_block:(b0 + nb) * wide_block])
        s.run_device(d_in, nb * wide_block, F, d_pow)
        d.run_device(d_pow, nb, d_rows, d_det)
        t.run_device(d_rows, d_det, nb, d_slots, d_blocks)
        z.set_track_table(d_slots, S, nb, bb, lag, 2)
        eng.accept_wideband_device(z, d_in, nb * wide_block, d_out, d_pcm, d_cnt)
        eng.synchronize()
        got = eng.dev_download(d_pcm, S * nb * bb // 64 * 2, np.int16).reshape(S, -1)
        cnt = eng.dev_download(d_cnt, 4 * S, np.uint32)
        slots = eng.dev_download(d_slots, 32 * nb * S).view(capi.TRACK_SLOT).reshape(nb, S)
        dec = [[(1, int(q["phase_inc"])) if q["state"] >= 2 else (0, 0) for q in slots[b]] for b in range(nb)]
        for b in range(nb):
            for c in range(S):
                live, inc = dec[b - lag][c] if b >= lag else carry[c]
                x = (inc - 2 ** 32 if inc >= 2 ** 31 else inc) / 4294967296.0 * rate
                hz = int(math.copysign(math.floor(abs(x) + 0.5), x))
                lines.append("%d %d %d 0x%08x %d" % (b_no + b, c, live, inc, hz))
        carry = dec[nb - 1]
        for c in range(S):
            pcm[c].append(got[c, :cnt[c]])
        b_no += nb
    assert (tmp_path / "track.log").read_text().splitlines() == lines
    for c in range(S):
        assert np.array_equal(np.fromfile(tmp_path / ("pcm_%d.s16" % c), np.int16), np.concatenate(pcm[c])), c
    assert {l.split()[2] for l in lines} == {"0", "1"} and len({l.split()[3] for l in lines}) > 3
    z.close()
    for o in (t, d, s):
        o.close()
    eng.close()
    tr = ["tracks=%d" % S, "bins=%d" % N, "frames=%d" % F]
    for extra in (["centre=100000000", "scan=99000000,101000000,100000"], ["agc=harris"], ["rxgain=20"],
                  ["decimation=75/8", "rate=2400000"], ["format=s8"], ["format=s16"]):
        r = subprocess.run(base + tr + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and len(r.stderr.strip().splitlines()) == 1 and "tracks=" in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + tr + ["lag=2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "usage" in r.stderr
