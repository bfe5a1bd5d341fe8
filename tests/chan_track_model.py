"""numpy model of track-following wideband channels (include/iqdemod.h: "Track-following channels").

A following channel's row is cut block by block: the table entry of the channel's source and slot for block b - lag (the
carry for block 0 at lag 1) decides whether the block is live and at which increment; a live block is
chan_model.channel(...) over the block's absolute outputs, any other 0x80.  The carry is state across calls.

DEFECTS are the ways a kernel can get this wrong; tests/test_chan_track_host.py proves that the inputs of the GPU test
(tests/chan_track_cases.py) tell each of them from the truth."""
import numpy as np

from tests import chan_model as cm

DEFECTS = (
    "late", "early",            # the table block read one late / one early
    "carry_dropped",            # the carry is not live at every call boundary
    "carry_over_reset",         # the carry survives reset
    "carry_at_start",           # the carry of a channel that has just started to follow counts
    "carry_lagged",             # the carry is taken from block n_blocks - 1 - lag instead of the last block
    "min_state_ignored",        # every slot with state >= 1 is live
    "closed_cut",               # a closing slot (state 0, track_id != 0) is cut
    "taps_held",                # the taps are those of the call's first block, the rotation moves on
    "rot_relative",             # rotation on the block-relative n
    "new_taps_old_rot",         # the block's taps with the previous block's rotation increment
    "old_taps_new_rot",         # and the reverse
    "source0",                  # the table row of source 0 for every channel
    "ch_as_slot",               # the channel index (mod S) used as the slot
    "silence_00",               # silence written as 0x00
    "bound_window",             # a block boundary rounded down to the window
    "bound_64",                 # a block boundary rounded down to 64 outputs
)


def _cut(wide_row, h, M, P, shift, m0, m1, d_taps, d_rot, origin):
    """outputs [m0, m1): taps from d_taps, rotation increment d_rot on n - origin M"""
    if d_taps == d_rot and origin == 0:
        return cm.channel(wide_row, h, M, d_taps, shift, P, m_range=(m0, m1))
    ar, ai = cm.channel(wide_row, h, M, d_taps, shift, P, m_range=(m0, m1), stage_a=True)
    n = (np.arange(m0, m1, dtype=np.int64) - origin) * M + M - 1
    idx = (((n.astype(np.uint64) * np.uint64(d_rot)) & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.int64)
    c, s = np.asarray(P, np.int64)[idx, 0], np.asarray(P, np.int64)[idx, 1]
    rr, ri = ar * c + ai * s, ai * c - ar * s
    L = int(shift)
    out = np.empty(2 * len(n), np.uint8)
    out[0::2] = (np.clip((rr + (1 << (21 - L))) >> (22 - L), -128, 127) + 128).astype(np.uint8)
    out[1::2] = (np.clip((ri + (1 << (21 - L))) >> (22 - L), -128, 127) + 128).astype(np.uint8)
    return out


class Follower:
    """One following channel: its carry and the outputs it has cut since create / reset."""

    def __init__(self, h, M, P, source, shift, slot, channel=0, defect=None, window=1024):
        self.h, self.M, self.P, self.source, self.shift, self.slot = h, int(M), P, int(source), int(shift), int(slot)
        self.channel, self.defect, self.window = int(channel), defect, int(window)
        self.carry = (False, 0)
        self.m_abs = 0

    def reset(self):
        if self.defect != "carry_over_reset":
            self.carry = (False, 0)
        self.m_abs = 0

    def start(self, slot=None):
        """the channel starts to follow (again), or moves to another slot"""
        if slot is not None:
            self.slot = int(slot)
        if self.defect != "carry_at_start":
            self.carry = (False, 0)

    def skip(self, n_out):
        """a call in which the channel did not follow"""
        self.m_abs += n_out

    def _decide(self, table, e, min_state, carry):
        """(live, d) of table block e of this channel's source and slot; e < 0: the carry"""
        if e < 0:
            return carry
        S = table.shape[2]
        t = table[0 if self.defect == "source0" else self.source, min(e, table.shape[1] - 1),
                  self.channel % S if self.defect == "ch_as_slot" else self.slot]
        state = int(t["state"])
        live = state >= (1 if self.defect == "min_state_ignored" else min_state)
        if self.defect == "closed_cut" and state == 0 and int(t["track_id"]) != 0:
            live = True
        return (True, int(t["phase_inc"])) if live else (False, 0)

    def call(self, wide_row, table, block_bytes, lag, min_state):
        """wide_row: the source's whole stream since create / reset (uint8), at least up to this call's end; table
        [n_sources][n_blocks][S] of capi.TRACK_SLOT.  Returns the call's row, n_blocks block_bytes bytes."""
        n_blocks, bo = table.shape[1], block_bytes // 2
        carry = (False, 0) if self.defect == "carry_dropped" else self.carry
        shiftb = {"late": -1, "early": 1}.get(self.defect, 0)
        dec = [self._decide(table, b - lag + shiftb, min_state, carry) for b in range(n_blocks)]
        first = dec[0]
        # the block an output is cut with: its own, or - the boundary defects - that of its window's / its 64's first output
        unit = {"bound_window": self.window if bo > self.window else 1, "bound_64": 64}.get(self.defect, 1)
        m = np.arange(n_blocks * bo)
        blk = np.minimum((m // unit * unit) // bo, n_blocks - 1)
        edges = [0] + [int(i) for i in np.nonzero(np.diff(blk))[0] + 1] + [len(m)]
        out = np.empty(2 * len(m), np.uint8)
        silence = 0x00 if self.defect == "silence_00" else 0x80
        for a, z in zip(edges[:-1], edges[1:]):
            b = int(blk[a])
            live, d = dec[b]
            prev = dec[b - 1] if b > 0 else carry
            if not live:
                out[2 * a:2 * z] = silence
                continue
            d_taps, d_rot, origin = d, d, 0
            if self.defect == "taps_held" and first[0]:
                d_taps = first[1]
            if self.defect == "rot_relative":
                origin = self.m_abs + a
            if self.defect == "new_taps_old_rot" and prev[0]:
                d_rot = prev[1]
            if self.defect == "old_taps_new_rot" and prev[0]:
                d_taps = prev[1]
            out[2 * a:2 * z] = _cut(wide_row, self.h, self.M, self.P, self.shift, self.m_abs + a, self.m_abs + z, d_taps, d_rot, origin)
        last = n_blocks - 1 - (lag if self.defect == "carry_lagged" else 0)
        self.carry = self._decide(table, last, min_state, carry) if last >= 0 else carry
        self.m_abs += n_blocks * bo
        return out
