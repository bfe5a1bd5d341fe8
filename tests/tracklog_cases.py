"""The inputs of the band track log's GPU test (tests/test_gpu_tracklog.py), built here so that the CPU tier can hold the very
same inputs to the mutation proof (tests/test_tracklog_host.py).  Everything is seeded; nothing here touches a GPU.

A case is one TrackLog object (a Cfg) and a script of calls: ("run", b0, b1) hands blocks b0 .. b1 - 1 of the case's slot and
measurement tables to one call, ("reset",) is iqd_tracklog_reset.  The tables are written by hand with Case.put and Case.life
at the smallest shapes that can go wrong.  Every byte the log does not read - all of a slot past track_id, state, width_class
and centre_q8, all of a free slot but its track_id, four fields of a measurement record, and all of a free slot's record - is
seeded garbage, so a kernel that read them would show.

The kernel gives a source to a wave and a slot to a lane, keeps the summaries in registers over a call and ranks a block's
events by a ballot, so the seams are S = 1 and 64, more than one source, calls of one block, and E."""
import numpy as np

from tests import measure_model as mm
from tests import track_model as tm
from tests import tracklog_model as lm

T, A, C = 1, 2, 0                                                        # a live slot's states; C with an id: its closing block


class Case:
    def __init__(self, name, cfg, n_blocks, calls=None, seed=0):
        lm.check_cfg(cfg)
        self.name, self.cfg, self.n_blocks = name, cfg, n_blocks
        self.calls = calls or [("run", 0, n_blocks)]
        J, S = cfg.n_sources, cfg.n_slots
        rng = np.random.default_rng([2000, seed])
        self.slots = np.ascontiguousarray(rng.integers(0, 256, (J, n_blocks, S, 32), dtype=np.uint8)).view(tm.SLOT_DTYPE).reshape(J, n_blocks, S)
        self.meas = np.ascontiguousarray(rng.integers(0, 256, (J, n_blocks, S, 32), dtype=np.uint8)).view(mm.MEAS_DTYPE).reshape(J, n_blocks, S)
        self.slots["track_id"] = 0

    def put(self, j, b, s, tid, state, hint=2, mflags=0, mid=None, centre=4000, cls=1, lo=10, hi=20, peak=100, esum=1000):
        """slot (j, b, s) holds track tid in `state` and its measurement record (track_id mid, left out: tid, as the
        measurement writes it; a closing block's record is zero bytes there)"""
        t, m = self.slots[j, b, s], self.meas[j, b, s]
        t["track_id"], t["state"], t["width_class"], t["centre_q8"] = tid, state, cls, centre
        if state == C and mid is None:
            self.meas[j, b, s] = np.zeros((), mm.MEAS_DTYPE)
            return
        m["track_id"], m["flags"], m["hint"] = tid if mid is None else mid, mflags, hint
        m["obw_lo"], m["obw_hi"], m["peak_excess"], m["sum_excess"] = lo, hi, peak, esum

    def life(self, j, s, b0, tid, states, hints=None, **kw):
        """consecutive blocks from b0: states is a list of T / A / C; hints a list (left out: NARROW throughout); a keyword
        may be a list with one value per block (a closing block at the end, whose record is zero bytes, needs none)"""
        for i, state in enumerate(states):
            last = state == C and i == len(states) - 1
            k = {n: ((0 if last and i == len(v) else v[i]) if isinstance(v, (list, tuple)) else v) for n, v in kw.items()}
            self.put(j, b0 + i, s, tid, state, hint=(0 if last and i == len(hints) else hints[i]) if hints else 2, **k)

    def freeze(self):
        self.slots.setflags(write=False)
        self.meas.setflags(write=False)
        return self

    def __repr__(self):
        return self.name


def run_script(case, log):
    """the case's calls on a log with run(slots, meas), reset() and state(source): a list with one (summary, events, counts)
    per run, and the final (summaries, g) of every source"""
    out = []
    for op in case.calls:
        if op[0] == "reset":
            log.reset()
        else:
            out.append(log.run(np.ascontiguousarray(case.slots[:, op[1]:op[2]]), np.ascontiguousarray(case.meas[:, op[1]:op[2]])))
    return out, [log.state(j) for j in range(case.cfg.n_sources)]


def model(case, defects=()):
    return run_script(case, lm.TrackLog(case.cfg, defects))


def same(got, want):
    """two run_script results, every byte"""
    (g_runs, g_state), (w_runs, w_state) = got, want
    if len(g_runs) != len(w_runs):
        return False
    for g, w in zip(g_runs, w_runs):
        if any(a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes() for a, b in zip(g, w)):
            return False
    return all(a[0].tobytes() == b[0].tobytes() and a[1] == b[1] for a, b in zip(g_state, w_state))


NAMES = ["S1-life", "S8-calls", "S8-calls-reset", "S8-votes", "S8-short-and-lost", "S8-E4-exact", "S8-E3-over", "S8-E1",
         "S64-burst", "S64-burst-E63", "J3-sources", "S4-tracker-reset", "N256-chained"]


def cfg(J=1, S=8, E=16, min_active=2, vote_min=4):
    return lm.Cfg(J, S, E, min_active, vote_min)


def _calls_table(c):
    """S = 8 over 12 blocks: what the call boundaries at 1, 4 and 7 can get wrong"""
    c.life(0, 0, 0, 1, [A, A, A, A, A, A, A, A, A, C], hints=[1, 1, 3, 3, 3, 3, 3, 2, 2, 2],                # lives across three calls and more
           centre=[4000 + 37 * i for i in range(10)], esum=[1000 + i for i in range(10)], peak=[90, 100, 80, 70, 60, 50, 40, 30, 20, 0],
           lo=[10, 9, 11, 12, 8, 10, 10, 10, 10, 0], hi=[20, 21, 19, 18, 25, 20, 20, 20, 20, 0])
    c.life(0, 1, 0, 2, [T, T, A, A, C])                                   # closes in a call's first block (4)
    c.life(0, 2, 0, 3, [A, A, A, C])                                      # closes in a call's last block (3)
    c.life(0, 2, 4, 7, [T, A, A, A, A, A, A, A], hints=[3] * 8, cls=[0, 1, 2, 3, 3, 3, 3, 3])   # the slot reused right behind its closing block
    c.life(0, 3, 0, 4, [C])                                               # a closing block is all the log ever sees of it
    c.life(0, 4, 3, 5, [A, C])                                            # one active block: short at min_active 2
    c.life(0, 5, 5, 6, [T, A, A, C], hints=[1, 1, 1, 1])                  # closes in the last block of its call (7) ... (8)
    c.life(0, 7, 6, 8, [A, A, A, A, A, A], centre=2 ** 19 - 1)            # still open at the end, the largest centre


def cases(P=None):
    """P: the phasor table ([4096, 2] int16, capi.channelizer_phasor_table()) for the chained case; without it that case is
    left out"""
    out = []

    # one slot: tentative, active, closed at 8, the slot reused by a new id in block 9; the vote reaches vote_min = 4 in
    # block 5 (tentative blocks vote too) at CARRIER 2 : NARROW 2 - a tie of two, the lowest hint - turns NARROW in block 6
    # and WIDE never; the closing block's record is zero bytes
    c = Case("S1-life", cfg(S=1, E=2), 12, seed=1)
    c.life(0, 0, 0, 1, [T, T, A, A, A, A, A, A, C], hints=[0, 1, 200, 1, 2, 2, 2, 3, 0], centre=[5000, 5010, 5020, 5100, 4900, 5000, 5050, 5060, 5060],
           esum=[2 ** 43 - 1, 5, 7, 2 ** 43 - 1, 9, 11, 13, 15, 0], peak=[2 ** 32 - 1, 5, 7, 100, 9, 11, 13, 15, 0],
           lo=[30, 31, 29, 40, 35, 35, 35, 35, 0], hi=[50, 49, 51, 45, 47, 47, 47, 65535, 0])
    c.life(0, 0, 9, 2, [A, A, A], hints=[3, 3, 3])
    out.append(c.freeze())

    c = Case("S8-calls", cfg(), 12, calls=[("run", 0, 1), ("run", 1, 4), ("run", 4, 7), ("run", 7, 8), ("run", 8, 12)], seed=2)
    _calls_table(c)
    out.append(c.freeze())
    # the same table with a reset of the log behind the second call: the tracks running then are seen as new ones
    c = Case("S8-calls-reset", cfg(), 12, calls=[("run", 0, 1), ("run", 1, 4), ("reset",), ("run", 4, 7), ("run", 7, 12)], seed=3)
    _calls_table(c)
    out.append(c.freeze())

    # the vote: per slot a different history of records over 8 active blocks and a closing one, vote_min = 3
    c = Case("S8-votes", cfg(vote_min=3, min_active=1), 9, seed=4)
    c.life(0, 0, 0, 1, [A] * 8 + [C], hints=[1, 2, 3, 1, 2, 3, 3, 0])     # a tie of three at V = 3 and at 6, then WIDE
    c.life(0, 1, 0, 2, [A] * 8 + [C], hints=[3, 2, 2, 3, 1, 1, 1, 1])     # NARROW, a tie of two (NARROW over WIDE), ... CARRIER
    c.life(0, 2, 0, 3, [A] * 8 + [C], hints=[0, 200, 2, 4, 255, 2, 0, 0]) # V = 2 < vote_min although n_measured = 8
    c.life(0, 3, 0, 4, [A] * 8 + [C], hints=[3] * 8, mflags=[0, 2, 2, 1, 0, 2, 1, 0])           # weak and empty records: V = 3 in the last block
    c.life(0, 4, 0, 5, [A] * 8 + [C], hints=[1] * 8, mid=[5, 4, 5, 0, 5, 6, 2 ** 32 - 1, 5],     # stale records: V = 4
           lo=[10, 1, 10, 10, 10, 10, 10, 10], hi=[20, 20, 20, 60000, 20, 20, 20, 20], peak=[100, 999, 100, 100, 100, 100, 100, 100])
    c.life(0, 5, 0, 6, [A] * 8 + [C], hints=[2, 2, 2, 1, 1, 1, 1, 3])     # NARROW, tied back to CARRIER, CARRIER
    c.life(0, 6, 0, 7, [T] * 8, hints=[3, 3, 1, 1, 1, 1, 2, 2])           # tentative throughout: votes, but never active; open at the end
    c.life(0, 7, 0, 8, [A] * 8 + [C], hints=[2] * 8, mflags=3, esum=0, peak=0)                  # never a vote: obw_lo_min stays 0xffff
    out.append(c.freeze())

    # what ends without being an event, and what ends lost: min_active = 3
    c = Case("S8-short-and-lost", cfg(min_active=3), 10, calls=[("run", 0, 3), ("run", 3, 10)], seed=5)
    c.life(0, 0, 0, 1, [T])                                               # a tentative slot dropped at its first miss: short
    c.life(0, 1, 0, 2, [T, T, A, A, C])                                   # 2 active blocks: short
    c.life(0, 1, 5, 9, [T, T, A, A, A, ])                                 # ... 3: open at the end
    c.life(0, 2, 0, 3, [A, A, A, C])                                      # exactly min_active: an event
    c.life(0, 3, 0, 4, [A, A, A])                                         # a foreign table: 4 is replaced by 5 without a closing
    c.life(0, 3, 3, 5, [A, A])                                            # block - LOST and NEW in one block, across the call boundary -
    c.life(0, 3, 5, 6, [A, A, A, A, A])                                   # and 5 by 6 with 2 active blocks: short
    c.life(0, 4, 1, 10, [A, A, A, A])                                     # vanishes to a free slot: LOST, 4 active
    c.life(0, 5, 2, 11, [T, A, A, A, T, A])                               # a state that goes back (foreign): counted as it comes
    c.life(0, 6, 0, 12, [A, A, A, A, A, A, A, C])
    c.life(0, 7, 8, 13, [C])                                              # an id first seen in its closing block, with a
    c.slots["state"][0, 0:8, 7] = 2                                       # free slot's state saying active before it
    out.append(c.freeze())

    # exactly E, E + 1, and E = 1: four tracks end in one call, three of them in one block
    for name, E in (("S8-E4-exact", 4), ("S8-E3-over", 3), ("S8-E1", 1)):
        c = Case(name, cfg(E=E), 6, calls=[("run", 0, 5), ("run", 5, 6)], seed=6)
        c.life(0, 1, 0, 1, [A, A, C])
        for s, tid in ((6, 2), (2, 3), (4, 4)):
            c.life(0, s, 0, tid, [A, A, A, C], centre=3000 + 100 * s)
        c.life(0, 4, 4, 7, [A, A])                                        # the second call has no event: its list is all zero
        c.life(0, 5, 1, 5, [A, C])                                        # short, between the events' slots
        out.append(c.freeze())

    # 64 slots, 64 events in one block - closed in the even slots, lost in the odd ones - with E = 64 and E = 63
    for name, E in (("S64-burst", 64), ("S64-burst-E63", 63)):
        c = Case(name, cfg(S=64, E=E, min_active=1, vote_min=1), 3, seed=7)
        for s in range(64):
            c.life(0, s, 0, 100 + s, [A, A] + ([C] if s % 2 == 0 else []), hints=[1 + s % 3] * 3, centre=1000 + 256 * s, esum=10 + s, peak=s)
        out.append(c.freeze())

    # three sources with different histories, two calls: state, g and the event lists are per source
    c = Case("J3-sources", cfg(J=3, S=8, E=2, min_active=1), 6, calls=[("run", 0, 3), ("run", 3, 6)], seed=8)
    c.life(0, 0, 0, 1, [A, A, A, A, C])
    c.life(1, 0, 0, 1, [A, C])
    c.life(1, 3, 1, 2, [A, A, A, A, A], hints=[3] * 5)
    c.life(1, 7, 0, 3, [A, A, C])
    c.life(1, 6, 0, 4, [A, A, C])
    c.life(2, 5, 2, 1, [T, A, A])
    c.life(2, 5, 5, 9, [A])
    out.append(c.freeze())

    # a tracker reset between two calls: the second call's table starts again with ids from 1 in the lowest slots, so slot
    # 0's id 1 is the same number and goes on (the log cannot tell), slot 1's differs (LOST and NEW), slot 2's track is gone
    c = Case("S4-tracker-reset", cfg(S=4, min_active=1), 8, calls=[("run", 0, 4), ("run", 4, 8)], seed=9)
    c.life(0, 0, 0, 1, [T, A, A, A])
    c.life(0, 1, 0, 3, [T, A, A, A])
    c.life(0, 2, 0, 2, [T, T, T, A])
    c.life(0, 0, 4, 1, [T, T, A, A])
    c.life(0, 1, 4, 2, [T, T, A, A])
    out.append(c.freeze())

    if P is not None:
        out.append(chained_case(P))
    assert [x.name for x in out] == (NAMES if P is not None else NAMES[:-1])
    return out


# The chained case: the keyed capture of tests/track_cases.py - an FM station at -700 kHz always on, an AM station at +250 kHz
# keyed on over blocks 6.5 .. 14.3 of 24 - through the spectrum, detector, tracker and measurement models into the log, in
# calls of 10, 10 and 4 blocks.
CHAINED_CALLS = [("run", 0, 10), ("run", 10, 20), ("run", 20, 24)]


def chained_tables(P):
    """(slots, meas) [1, 24, 4] of the chained capture from the four models, the tools' defaults"""
    from tests import detect_cases as dc
    from tests import detect_model as dm
    from tests import spectrum_model as sm
    from tests import track_cases as tc
    k = tc.CHAINED
    N, F, nb, S = k["N"], k["F"], k["blocks"], k["S"]
    power = sm.spectrum(tc.chained_wide(), "u8", N, F, None, P)[0]
    rows, det = dm.detect(power, dc.readme_cfg(N))
    slots, _ = tm.Tracker(tc.chained_cfg()).run(rows.reshape(1, nb), det.reshape(1, nb, 16))
    wide = max(N // 32, 2)
    mcfg = mm.Cfg(1, N, S, 1, max(N // 256, 1), 328, 1, 4096, 160, wide)      # capi.measure_defaults(N)
    meas = mm.measure(power.reshape(1, nb, N), rows.reshape(1, nb), slots, mcfg)
    return slots, meas


def chained_case(P):
    from tests import track_cases as tc
    c = Case("N256-chained", cfg(S=tc.CHAINED["S"], E=256, min_active=2, vote_min=4), tc.CHAINED["blocks"], calls=CHAINED_CALLS, seed=10)
    c.slots, c.meas = chained_tables(P)
    return c.freeze()


# The seeded slice of random scripts: case i of seed s is default_rng([s, i]).
FUZZ_SEED, FUZZ_CASES = 20261, 200
HINTS = [0, 1, 1, 2, 2, 3, 3, 200]


def random_case(seed, i):
    """S from {1, 5, 64}, 1 .. 3 sources, 1 .. 4 calls of 1 .. 9 blocks, now and then a reset between them; per slot ids are
    opened, promoted, closed, lost (to a free slot or to another id) and reused at random; E is drawn small enough to overflow"""
    rng = np.random.default_rng([seed, i])
    S = int(rng.choice([1, 5, 64]))
    J = int(rng.integers(1, 4))
    lens = [int(rng.integers(1, 10)) for _ in range(int(rng.integers(1, 5)))]
    calls, b = [], 0
    for n in lens:
        if calls and rng.random() < 0.1:
            calls.append(("reset",))
        calls.append(("run", b, b + n))
        b += n
    E = int(rng.integers(1, 4)) if S < 64 else int(rng.choice([1, 3, 20, 64]))
    c = Case("fuzz-%d-%d" % (seed, i), lm.Cfg(J, S, E, int(rng.integers(1, 4)), int(rng.integers(1, 5))), b, calls, seed=i)
    p_open, p_end = (0.5, 0.3) if S < 64 else (0.3, 0.25)
    for j in range(J):
        next_id = 0
        for s in range(S):
            tid, state = 0, 0
            for blk in range(b):
                r = rng.random()
                if tid == 0:
                    if r < p_open:
                        next_id += 1
                        tid, state = next_id * 64 + s, int(rng.choice([T, A]))
                elif r < p_end / 2:                                       # the closing block
                    c.put(j, blk, s, tid, C)
                    tid = 0
                    continue
                elif r < p_end * 3 / 4:                                   # lost to a free slot
                    tid = 0
                elif r < p_end:                                           # lost to another id
                    next_id += 1
                    tid, state = next_id * 64 + s, int(rng.choice([T, A]))
                elif state == T and r < 0.7:
                    state = A
                if tid:
                    esum = int(rng.integers(1, 2 ** 43))
                    lo = int(rng.integers(0, 2048))
                    c.put(j, blk, s, tid, state, hint=int(rng.choice(HINTS)), mflags=int(rng.choice([0, 0, 0, 0, 1, 2])),
                          mid=None if rng.random() < 0.9 else tid + 1, centre=int(rng.integers(0, 2 ** 19)), cls=int(rng.integers(0, 4)),
                          lo=lo, hi=int(rng.integers(lo, 2048)), peak=int(rng.integers(1, min(esum, 2 ** 32 - 1) + 1)), esum=esum)
    return c.freeze()


def fuzz_cases():
    return [random_case(FUZZ_SEED, i) for i in range(FUZZ_CASES)]


def kinds(case, result):
    """which of the four things the host test counts a fuzz case holds: a call that overflows E, a LOST event, a decision on
    a tie of votes, a track that spans a call boundary"""
    runs, _ = result
    found = set()
    vm = case.cfg.vote_min
    prev = None
    ops = [op for op in case.calls]
    r = 0
    for op in ops:
        if op[0] == "reset":
            prev = None
            continue
        summary, events, counts = runs[r]
        r += 1
        if (counts["n_events"] > counts["n_stored"]).any():
            found.add("overflow")
        if counts["n_lost"].any():
            found.add("lost")
        v = summary["votes"].astype(np.int64)
        top = v.max(axis=-1)
        if ((v.sum(axis=-1) >= vm) & ((v == top[..., None]).sum(axis=-1) >= 2) & (summary["track_id"] != 0)).any():
            found.add("tie")
        if prev is not None:
            first = summary[:, 0, :]
            if ((first["track_id"] != 0) & (first["track_id"] == prev["track_id"]) & (prev["state"] != 0) & ((first["flags"] & lm.F_NEW) == 0)).any():
                found.add("span")
        prev = summary[:, -1, :]
    return found
