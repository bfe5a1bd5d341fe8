"""The inputs of tests/test_gpu_chan_track.py (track-following wideband channels), the smallest that reach every path of
chz_track_kernel; tests/test_chan_track_host.py proves on the numpy model (tests/chan_track_model.py) that they expose the
model's defects.  Nothing here needs a GPU.

A case is one channelizer, a slot table of ncalls x nblk blocks per source (ncalls is 3 but for the one-block calls) and a script: ("run", t) is one call of nblk blocks
with table piece t (blocks [t nblk, (t + 1) nblk)) on the next piece of the capture, ("reset",) iqd_channelizer_reset (the
capture starts again), ("stop", channels) / ("start", channels) iqd_channelizer_follow_tracks with -1 / the channel's slot."""
import collections

import numpy as np

from rtlsdrdiags_amd.capi import TRACK_SLOT

Case = collections.namedtuple("Case", "name M taps h n_src wide src inc shift slot S bb nblk ncalls lag min_state table script")
# taps: what the channelizer is created with (None: its default taps), h: the taps themselves; wide [n_src, bytes]: ncalls
# calls' worth; slot [n_ch]: the table slot the channel follows, -1: a fixed channel (increment inc, as the followers have
# while they are stopped); bb: the table's block_bytes; table [n_src][ncalls nblk][S] TRACK_SLOT

ENGINE_BB = 256                                   # the engine's own block_bytes in every case: every call's row is a multiple
RUNS = [("run", 0), ("run", 1), ("run", 2)]
SPECIAL = (0, 0x80000000, 0xffffffff)
FREE, TENTATIVE, ACTIVE, CLOSING = range(4)


def k300_taps():
    """300 taps at M = 8 (10 K-chunks: more than stay in registers), a Hamming-windowed sinc of DC gain 32768"""
    x = np.arange(300) - 149.5
    w = np.sinc(2 * 0.06 * x) * np.hamming(300)
    h = np.rint(w / w.sum() * 32768).astype(np.int64)
    h[150] += 32768 - h.sum()
    return h.astype(np.int16)


def kind_of(t):
    """FREE, TENTATIVE, ACTIVE or CLOSING of table entries"""
    return np.where(t["state"] == 2, ACTIVE, np.where(t["state"] == 1, TENTATIVE, np.where(t["track_id"] != 0, CLOSING, FREE)))


def synthetic_table(rng, n_src, n_blocks, S, nblk):
    """Every entry drawn on its own: free (all-zero bytes), tentative, active or closing (state 0, the rest kept), the
    increment new in every block - 0, 0x80000000 and 0xffffffff among them - and every field the channelizer must not read
    random.  The last block of every call of nblk > 1 blocks is mostly active, so that carries are live."""
    raw = rng.integers(0, 256, (n_src, n_blocks, S, TRACK_SLOT.itemsize), dtype=np.uint8)
    t = np.ascontiguousarray(raw).view(TRACK_SLOT).reshape(n_src, n_blocks, S).copy()
    kind = rng.choice(4, size=t.shape, p=[0.15, 0.2, 0.5, 0.15])
    for b in range(n_blocks):
        if nblk > 1 and b % nblk == nblk - 1:
            kind[:, b] = np.where(rng.random((n_src, S)) < 0.8, ACTIVE, kind[:, b])
    t["state"] = np.where(kind == ACTIVE, 2, np.where(kind == TENTATIVE, 1, 0))
    t["track_id"] = np.where(kind == FREE, 0, t["track_id"] | 1)
    sp = rng.random(t.shape) < 0.12
    t["phase_inc"] = np.where(sp, np.asarray(SPECIAL, np.uint32)[rng.integers(0, 3, t.shape)], t["phase_inc"])
    t[kind == FREE] = np.zeros((), TRACK_SLOT)
    return t


def channel_plan(rng, n_follow, n_fixed, follow_sources, fixed_sources, S):
    """Followers and fixed channels interleaved; followers take slots so that slot != channel mod S for most, and the first
    two followers of a source share a slot when there are at least two."""
    n = n_follow + n_fixed
    src, inc, shift = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    slot = np.full(n, -1, np.int32)
    order = rng.permutation(n)
    shared = {}
    for i, c in enumerate(order):
        inc[c] = int(rng.integers(0, 2 ** 32))
        if i < n_follow:
            src[c] = follow_sources[i % len(follow_sources)]
            k = i // len(follow_sources)
            slot[c] = (int(c) + 1 + k) % S
            if k == 0:
                shared[int(src[c])] = int(slot[c])
            elif k == 1:
                slot[c] = shared[int(src[c])]     # two channels on one slot
            shift[c] = 8 - i % 9
        else:
            src[c] = fixed_sources[i % len(fixed_sources)]
            shift[c] = i % 9
    return src, inc, shift, slot


def chained(capi, P):
    """The keyed capture of tests/track_cases.py's chained case through the spectrum, detector and tracker models into the
    table: M = 8, a table block is 2 N F = 4096 wide bytes, 512 row bytes; 24 blocks in three calls.  One channel per slot."""
    from tests import detect_cases as dc
    from tests import detect_model as dm
    from tests import spectrum_model as sm
    from tests import track_cases as tc
    from tests import track_model as tm
    c = tc.CHAINED
    wide = tc.chained_wide()
    power = sm.spectrum(wide, "u8", c["N"], c["F"], None, P)[0]
    rows, det = dm.detect(power, dc.readme_cfg(c["N"]))
    slots, _ = tm.Tracker(tc.chained_cfg()).run(rows.reshape(1, -1), det.reshape(1, c["blocks"], 16))
    table = np.ascontiguousarray(slots).view(TRACK_SLOT).reshape(1, c["blocks"], c["S"])
    M = tc.RATE // 256000
    n = c["S"]
    return Case("M8-chained", M, None, capi.channelizer_default_taps(M), 1, wide, np.zeros(n, np.uint32), np.zeros(n, np.uint64),
                np.full(n, 2, np.uint8), np.arange(n, dtype=np.int32), c["S"], 2 * c["N"] * c["F"] // M, c["blocks"] // 3, 3, 0, 2,
                table, RUNS)


def case_names():
    return ["M8-1f-S1-b64", "M8-7f-S8-b256-script", "M2-9f-S8-b256", "M7-65f-S64-b1024", "K300-9f-S8-b256", "M8-9f-S8-b2560",
            "M8-7f-S8-b256-1blk", "M8-chained"]


def cases(capi, P):
    out = []
    script = [("run", 0), ("run", 1), ("reset",), ("run", 2), ("stop", "some"), ("run", 0), ("start", "some"), ("run", 1)]
    #     name                      M  K   follow fixed src follow on  fixed on  S   bb   nblk lag min_state script
    rows = (("M8-1f-S1-b64", 8, None, 1, 2, 1, [0], [0], 1, 64, 12, 0, 2, RUNS),
            ("M8-7f-S8-b256-script", 8, None, 7, 2, 1, [0], [0], 8, 256, 3, 1, 2, script),
            ("M2-9f-S8-b256", 2, None, 9, 3, 3, [0, 2], [1], 8, 256, 12, 1, 1, RUNS),
            ("M7-65f-S64-b1024", 7, None, 65, 4, 3, [0, 1, 2], [1], 64, 1024, 3, 0, 1, RUNS),
            ("K300-9f-S8-b256", 8, 300, 9, 2, 1, [0], [0], 8, 256, 3, 1, 2, RUNS),
            ("M8-9f-S8-b2560", 8, None, 9, 0, 1, [0], [0], 8, 2560, 3, 1, 2, RUNS),
            ("M8-7f-S8-b256-1blk", 8, None, 7, 1, 1, [0], [0], 8, 256, 1, 1, 2, [("run", t) for t in range(12)]))
    for i, (name, M, K, nf, nx, n_src, fs_on, fx_on, S, bb, nblk, lag, ms, scr) in enumerate(rows):
        rng = np.random.default_rng(300 + i)
        taps = None if K is None else k300_taps()
        h = capi.channelizer_default_taps(M) if taps is None else taps
        ncalls = 1 + max(op[1] for op in scr if op[0] == "run")
        wide = rng.integers(0, 256, (n_src, ncalls * nblk * bb * M), dtype=np.uint8)   # random bytes over the whole range
        wide[0, 64:72] = [0, 255, 255, 0, 0, 0, 255, 255]
        src, inc, shift, slot = channel_plan(rng, nf, nx, fs_on, fx_on, S)
        table = synthetic_table(rng, n_src, ncalls * nblk, S, nblk)
        fol = np.nonzero(slot >= 0)[0]
        for j, inc_sp in enumerate(SPECIAL):       # the three special increments in live blocks of followed positions
            ch, blk = fol[j % len(fol)], (1 + 2 * j) % (ncalls * nblk)
            table[src[ch], blk, slot[ch]] = (2 * j + 1, 2, 0, 3, 0, 0, 5, 0, inc_sp, 1, 2, 3, 4)
        if S == 1:                                 # one slot: every kind in turn, active at the calls' ends
            k = np.array(([ACTIVE, TENTATIVE, ACTIVE, FREE, CLOSING, ACTIVE] * 6)[:3 * nblk])
            table["state"][0, :, 0] = np.where(k == ACTIVE, 2, np.where(k == TENTATIVE, 1, 0))
            table["track_id"][0, :, 0] = np.where(k == FREE, 0, 7)
            table["phase_inc"][0, :, 0] = rng.integers(0, 2 ** 32, 3 * nblk, dtype=np.uint64)
            table["phase_inc"][0, 2::12, 0], table["phase_inc"][0, 5::12, 0], table["phase_inc"][0, 8::12, 0] = SPECIAL
        table.setflags(write=False)
        wide.setflags(write=False)
        out.append(Case(name, M, taps, h, n_src, wide, src, inc, shift, slot, S, bb, nblk, ncalls, lag, ms, table, scr))
    out.append(chained(capi, P))
    assert [c.name for c in out] == case_names()
    return out


def some(case):
    """the channels a script stops and starts: every second follower"""
    return [int(c) for c in np.nonzero(case.slot >= 0)[0][::2]]


def window_of(capi, case):
    """outputs of one window of a follower's block: the channelizer's window less the prototype's LDS share"""
    return min(capi.channelizer_window_outputs(case.M, len(case.h)), capi.channelizer_track_window_outputs(case.M, len(case.h)))


def run_model(tm, cm, case, P, c, defect=None, window=1024, script=None):
    """Channel c of a case through its script on the model: the rows of the script's runs, a list"""
    f = tm.Follower(case.h, case.M, P, case.src[c], case.shift[c], case.slot[c], channel=c, defect=defect, window=window)
    following, pos, out = case.slot[c] >= 0, 0, []
    span = case.nblk * case.bb * case.M
    for op in script or case.script:
        if op[0] == "reset":
            f.reset()
            pos = 0
        elif op[0] in ("stop", "start"):
            if case.slot[c] >= 0 and c in (some(case) if op[1] == "some" else op[1]):
                following = op[0] == "start"
                if following:
                    f.start()
        else:
            wide_row = case.wide[case.src[c], :(pos + 1) * span]
            if following:
                out.append(f.call(wide_row, case.table[:, op[1] * case.nblk:(op[1] + 1) * case.nblk], case.bb, case.lag, case.min_state))
            else:
                m0 = pos * case.nblk * case.bb // 2
                out.append(cm.channel(wide_row, case.h, case.M, int(case.inc[c]), int(case.shift[c]), P,
                                      m_range=(m0, m0 + case.nblk * case.bb // 2)))
                f.skip(case.nblk * case.bb // 2)
            pos += 1
    return out
