"""numpy int64 model of the fractional-rate channelizer's integer spec (include/iqdemod.h: "Fractional decimation").

Decimation P / Q: output m has u = m P + P - 1, n = u // Q (the newest wide sample it uses) and the tap set of branch
r = u % Q, h_r[k] = h[k Q + r].  Everything after the choice of (n, r) is chan_model's arithmetic.  The GPU's bytes must
equal these exactly.  `mutant` switches on one defect a kernel or its host side could plausibly have; mutant=None is the
spec (tests/test_chan_frac_host.py holds every GPU input to showing each of them)."""
import numpy as np

from tests import chan_model as cm

MUTANTS = (
    "branch_plus_1",      # r = (u + 1) mod Q
    "branch_reversed",    # branch Q - 1 - r
    "n_ceil",             # n = ceil(u / Q)
    "phasor_neighbour",   # the rotation phasor taken at the n of output m - 1
    "delay_q_grid",       # i_k from k Q + r: the tap delays counted on the prototype's grid
    "call_restart",       # a later call restarts its residue sequence one output early (needs `calls`)
)


def branches(h, Q):
    """[h_0, .., h_{Q-1}] int64; a branch may be empty."""
    h = np.asarray(h, np.int64)
    return [h[r::Q] for r in range(Q)]


def branch_taps(hr, r, Q, inc, Ptab, mutant=None):
    """(gr, gi) of one branch on its own sample delays k (the mutant: on k Q + r)."""
    k = np.arange(len(hr), dtype=np.uint64)
    if mutant == "delay_q_grid":
        k = k * np.uint64(Q) + np.uint64(r)
    idx = (((k * np.uint64(inc)) & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.int64)
    Pt = np.asarray(Ptab, np.int64)
    return (hr * Pt[idx, 0] + (1 << 14)) >> 15, (hr * Pt[idx, 1] + (1 << 14)) >> 15


def schedule(m, P, Q, mutant=None, calls=None):
    """(n, r, n_phasor) of the outputs m (int64 array).  calls: the outputs at which a call begins (for call_restart)."""
    m = np.asarray(m, np.int64)
    mm = m
    if mutant == "call_restart":
        later = np.zeros(len(m), bool)
        for b in (calls or ()):
            if b > 0:
                later |= m >= b
        mm = m - later.astype(np.int64)
    u = mm * P + P - 1
    n = -((-u) // Q) if mutant == "n_ceil" else u // Q
    r = u % Q
    if mutant == "branch_plus_1":
        r = (u + 1) % Q
    elif mutant == "branch_reversed":
        r = Q - 1 - r
    n_ph = ((mm - 1) * P + P - 1) // Q if mutant == "phasor_neighbour" else n
    return n, r, n_ph


def source_windows(wide_row, n, kb):
    """[len(n), kb, 2] int64: x[n_j], x[n_j - 1], .. x[n_j - kb + 1] (newest first), x[< 0] = 0, x past the end = 0."""
    u = np.asarray(wide_row, np.int64).reshape(-1, 2) - 128
    x = np.zeros((kb - 1 + len(u) + 1, 2), np.int64)      # (one zero behind for the n_ceil mutant's last output)
    x[kb - 1:kb - 1 + len(u)] = u
    if kb == 0 or len(n) == 0:
        return np.zeros((len(n), 0, 2), np.int64)
    win = np.lib.stride_tricks.sliding_window_view(x, kb, axis=0)     # [pos, 2, kb], oldest first
    return win[np.asarray(n, np.int64)][:, :, ::-1].transpose(0, 2, 1)


def channels(wide_row, h, P, Q, incs, shifts, Ptab, m_range=None, mutant=None, calls=None):
    """The output bytes [len(incs), 2 (m1 - m0)] of every channel (inc, shift) of one source: wide_row is that source's
    whole stream from sample 0 (uint8), m_range the outputs wanted (default: all the stream gives)."""
    n_wide = len(wide_row) // 2
    m0, m1 = (0, n_wide * Q // P) if m_range is None else m_range
    m = np.arange(m0, m1, dtype=np.int64)
    n, r, n_ph = schedule(m, P, Q, mutant, calls)
    br = branches(h, Q)
    Pt = np.asarray(Ptab, np.int64)
    out = np.empty((len(incs), 2 * len(m)), np.uint8)
    A = np.zeros((2, len(incs), len(m)), np.int64)
    for rr in range(Q):
        sel = np.nonzero(r == rr)[0]
        hr = br[rr]
        if len(sel) == 0 or len(hr) == 0:
            continue
        w = source_windows(wide_row, n[sel], len(hr))
        wr, wi = w[:, :, 0], w[:, :, 1]
        for c, inc in enumerate(incs):
            gr, gi = branch_taps(hr, rr, Q, inc, Ptab, mutant)
            A[0, c, sel] = wr @ gr - wi @ gi
            A[1, c, sel] = wi @ gr + wr @ gi
    for c, (inc, L) in enumerate(zip(incs, shifts)):
        ar = np.clip((A[0, c] + 128) >> 8, -32768, 32767)
        ai = np.clip((A[1, c] + 128) >> 8, -32768, 32767)
        idx = (((n_ph.astype(np.uint64) * np.uint64(inc)) & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.int64)
        cc, ss = Pt[idx, 0], Pt[idx, 1]
        r_r, r_i = ar * cc + ai * ss, ai * cc - ar * ss
        L = int(L)
        out[c, 0::2] = (np.clip((r_r + (1 << (21 - L))) >> (22 - L), -128, 127) + 128).astype(np.uint8)
        out[c, 1::2] = (np.clip((r_i + (1 << (21 - L))) >> (22 - L), -128, 127) + 128).astype(np.uint8)
    return out


def channel(wide_row, h, P, Q, inc, shift, Ptab, m_range=None, mutant=None, calls=None):
    """One channel's bytes: chan_model.channel's arguments with the denominator Q after the numerator P."""
    return channels(wide_row, h, P, Q, [inc], [shift], Ptab, m_range, mutant, calls)[0]


def channelize(wide, h, P, Q, sources, incs, shifts, Ptab, m_range=None, mutant=None, calls=None):
    """All channels: wide [n_sources, bytes] -> [n_ch, bytes Q / P] (or the outputs of m_range)."""
    wide = np.asarray(wide).reshape(-1, np.asarray(wide).shape[-1])
    sources = np.asarray(sources, np.int64)
    rows = [None] * len(sources)
    for s in np.unique(sources):
        at = np.nonzero(sources == s)[0]
        got = channels(wide[s], h, P, Q, [incs[i] for i in at], [shifts[i] for i in at], Ptab, m_range, mutant, calls)
        for j, i in enumerate(at):
            rows[i] = got[j]
    return np.stack(rows)
