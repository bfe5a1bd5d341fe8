"""Band track log (include/iqdemod.h: "Band track log") as a plain model written from the header's text and not from the
kernel: one Python dict per (source, slot), worked block by block and slot by slot in order - no lanes, no ballots, no ranks.
`defects` switches on ways this can go wrong (one name or several); the CPU tier (tests/test_tracklog_host.py) shows that the
GPU test's inputs (tests/tracklog_cases.py) see each of them.  Without a defect the model asserts every bound the header states
on every entry it reads or writes."""
from collections import namedtuple

import numpy as np

from tests import measure_model as mm
from tests import track_model as tm

F_NEW, F_MODE_CHANGED, F_CLOSED, F_LOST = 1, 2, 4, 8
M32, M64 = 2 ** 32 - 1, 2 ** 64 - 1

SUMMARY_DTYPE = np.dtype([("track_id", "<u4"), ("state", "u1"), ("flags", "u1"), ("mode_hint", "u1"), ("width_class", "u1"),
                          ("first_block", "<u8"), ("n_blocks", "<u4"), ("n_active", "<u4"), ("n_measured", "<u4"),
                          ("votes", "<u4", (3,)), ("sum_centre_q8", "<u8"), ("sum_excess", "<u8"), ("peak_excess", "<u4"),
                          ("obw_lo_min", "<u2"), ("obw_hi_max", "<u2")])
COUNTS_DTYPE = np.dtype([("n_events", "<u4"), ("n_stored", "<u4"), ("n_short", "<u4"), ("n_lost", "<u4")])
assert SUMMARY_DTYPE.itemsize == 64 and COUNTS_DTYPE.itemsize == 16

Cfg = namedtuple("Cfg", "n_sources n_slots max_events min_active vote_min")

DEFECTS = [
    "weak_votes",             # a weak record votes
    "stale_votes",            # a record whose track_id is not the slot's votes
    "tie_high",               # a tie of votes goes to the highest hint
    "vote_min_measured",      # vote_min is compared with n_measured, not with the sum of the votes
    "mode_sticky",            # mode_hint is never revised after the first decision
    "tentative_active",       # n_active counts tentative blocks too
    "centre_all_live",        # sum_centre_q8 runs over all live blocks
    "first_block_rel",        # first_block is the block's index in its call
    "state_dropped",          # the summaries are dropped at a call boundary
    "reset_kept",             # reset keeps the state
    "closing_counted",        # the closing block counts in n_blocks
    "lost_silent",            # a vanished track is neither an event nor short
    "events_descending",      # the events of a block in descending slot order
    "events_clipped",         # n_events is clipped to E
    "min_active_off",         # an event needs more than min_active active blocks
    "lost_unflagged",         # a lost event lacks its flag and its count
    "closed_kept",            # a closed summary is not zeroed: the slot's next track inherits it
    "g_per_call",             # the block index advances once per call
]


def check_cfg(c):
    assert c.n_sources >= 1 and 1 <= c.n_slots <= 64 and 1 <= c.max_events <= 65536
    assert 1 <= c.min_active <= 65535 and 1 <= c.vote_min <= 65535


def _free():
    return dict(track_id=0, state=0, flags=0, mode_hint=0, width_class=0, first_block=0, n_blocks=0, n_active=0, n_measured=0,
                votes=[0, 0, 0], sum_centre_q8=0, sum_excess=0, peak_excess=0, obw_lo_min=0, obw_hi_max=0)


def _record(st):
    return tuple(tuple(st[n]) if n == "votes" else st[n] for n in SUMMARY_DTYPE.names)


def decide(votes, vote_min, tie_high=False):
    """step 3 on three vote counts: 0 under vote_min votes, otherwise the hint with the most, a tie to the lowest"""
    if (sum(votes) & M32) < vote_min:
        return 0
    top = max(votes)
    at = [i + 1 for i in range(3) if votes[i] == top]
    return at[-1] if tie_high else at[0]


class TrackLog:
    def __init__(self, cfg, defects=()):
        check_cfg(cfg)
        self.cfg = cfg
        self.df = (defects,) if isinstance(defects, str) else tuple(defects or ())
        assert all(x in DEFECTS for x in self.df), self.df
        self._zero()

    def _zero(self):
        self.g = [0] * self.cfg.n_sources
        self.st = [[_free() for _ in range(self.cfg.n_slots)] for _ in range(self.cfg.n_sources)]

    def reset(self):
        if "reset_kept" not in self.df:
            self._zero()

    def state(self, source=0):
        out = np.zeros(self.cfg.n_slots, SUMMARY_DTYPE)
        for s, st in enumerate(self.st[source]):
            out[s] = _record(st)
        return out, self.g[source]

    def run(self, slots, meas):
        """slots [n_sources, n_blocks, S] (track_model.SLOT_DTYPE), meas [n_sources, n_blocks, S] (measure_model.MEAS_DTYPE)
        -> summary [n_sources, n_blocks, S], events [n_sources, E], counts [n_sources]"""
        c, df = self.cfg, self.df
        slots, meas = np.asarray(slots), np.asarray(meas)
        assert slots.dtype == tm.SLOT_DTYPE and meas.dtype == mm.MEAS_DTYPE
        J, S, E = c.n_sources, c.n_slots, c.max_events
        B = slots.shape[1]
        assert slots.shape == (J, B, S) and meas.shape == (J, B, S) and B >= 1 and J * B <= 2 ** 31 - 1
        summary = np.zeros((J, B, S), SUMMARY_DTYPE)
        events = np.zeros((J, E), SUMMARY_DTYPE)
        counts = np.zeros(J, COUNTS_DTYPE)
        need = c.min_active + 1 if "min_active_off" in df else c.min_active
        for j in range(J):
            if "state_dropped" in df:
                self.st[j] = [_free() for _ in range(S)]
            found, n_short, n_lost = [], 0, 0
            for b in range(B):
                of_block = []
                for s in range(S):
                    t, m, st = slots[j, b, s], meas[j, b, s], self.st[j][s]
                    tid, tstate = int(t["track_id"]), int(t["state"])
                    if not df and tid != 0:                          # (of a slot without an id nothing else is read)
                        assert tstate <= 2 and int(t["width_class"]) <= 3 and int(t["centre_q8"]) < 2 ** 19
                    st["flags"] = 0
                    # 0 vanished
                    if st["track_id"] != 0 and tid != st["track_id"]:
                        if "lost_silent" not in df:
                            if st["n_active"] >= need:
                                ev = dict(st, votes=list(st["votes"]), flags=0 if "lost_unflagged" in df else F_LOST)
                                of_block.append(_record(ev))
                                n_lost += "lost_unflagged" not in df
                            else:
                                n_short += 1
                        st = self.st[j][s] = _free()
                    # 1 start
                    if tid != 0 and st["track_id"] == 0:
                        st.update(track_id=tid, first_block=b if "first_block_rel" in df else self.g[j], obw_lo_min=0xffff)
                        st["flags"] |= F_NEW
                    if st["track_id"] != 0:
                        before = st["mode_hint"]
                        # 2 accumulate
                        if tstate != 0 or "closing_counted" in df:
                            st["n_blocks"] = (st["n_blocks"] + 1) & M32
                        if tstate != 0:
                            st["state"], st["width_class"] = tstate, int(t["width_class"])
                            if tstate == 2 or "tentative_active" in df:
                                st["n_active"] = (st["n_active"] + 1) & M32
                            if tstate == 2 or "centre_all_live" in df:
                                st["sum_centre_q8"] += int(t["centre_q8"])
                            mflags = int(m["flags"])
                            if "weak_votes" in df:
                                mflags &= ~mm.F_WEAK
                            if (int(m["track_id"]) == tid or "stale_votes" in df) and mflags == 0:
                                assert df or (int(m["sum_excess"]) < 2 ** 43 and int(m["peak_excess"]) <= int(m["sum_excess"]))
                                st["n_measured"] = (st["n_measured"] + 1) & M32
                                st["sum_excess"] = (st["sum_excess"] + int(m["sum_excess"])) & M64
                                st["peak_excess"] = max(st["peak_excess"], int(m["peak_excess"]))
                                st["obw_lo_min"] = min(st["obw_lo_min"], int(m["obw_lo"]))
                                st["obw_hi_max"] = max(st["obw_hi_max"], int(m["obw_hi"]))
                                if 1 <= int(m["hint"]) <= 3:
                                    st["votes"][int(m["hint"]) - 1] = (st["votes"][int(m["hint"]) - 1] + 1) & M32
                        # 3 decide
                        votes = st["votes"]
                        if "vote_min_measured" in df:
                            mode = 0 if st["n_measured"] < c.vote_min else decide(votes, 0)
                        else:
                            mode = decide(votes, c.vote_min, "tie_high" in df)
                        if "mode_sticky" in df and before != 0:
                            mode = before
                        if mode != before:
                            st["flags"] |= F_MODE_CHANGED
                        st["mode_hint"] = mode
                        if not df:
                            assert st["sum_centre_q8"] < 2 ** 51 and st["n_active"] <= st["n_blocks"] and sum(votes) <= st["n_measured"] <= st["n_blocks"]
                            assert st["n_measured"] == 0 or st["obw_lo_min"] <= st["obw_hi_max"]
                        # 4 close
                        if tstate == 0:
                            st["flags"] |= F_CLOSED
                            st["state"] = 0
                            if st["n_active"] >= need:
                                of_block.append(_record(st))
                            else:
                                n_short += 1
                    summary[j, b, s] = _record(st)
                    if st["flags"] & F_CLOSED and "closed_kept" not in df:
                        self.st[j][s] = _free()
                found += of_block[::-1] if "events_descending" in df else of_block
                if "g_per_call" not in df:
                    self.g[j] += 1
            if "g_per_call" in df:
                self.g[j] += 1
            for i, ev in enumerate(found[:E]):
                events[j, i] = ev
            n_events = min(len(found), E) if "events_clipped" in df else len(found)
            counts[j] = (n_events & M32, min(len(found), E), n_short & M32, n_lost & M32)
        return summary, events, counts
