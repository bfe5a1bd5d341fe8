"""numpy model of the channelizer's band survey (include/iqdemod.h: "Band survey").

Entry (s, b, p) is the block magnitude of SignalDetector - the oracle's block_magnitude, the reference-pinned one - over
block b of the row that a channel (source s, d_p, L_p) gets from the existing integer spec: chan_model.channel for an
integer decimation, chan_frac_model.channels for P / Q.  The GPU's numbers must equal these exactly.  `mutant` switches on
one defect a survey kernel or its host side could plausibly have; mutant=None is the spec
(tests/test_chan_survey_host.py holds every GPU input to showing each of them)."""
import numpy as np

from tests import chan_frac_model as fm
from tests import chan_model as cm

MUTANTS = (
    "abs_127",          # |-128| taken as 127
    "mean_ab",          # (a + b) >> 1 instead of max + (min >> 1)
    "boundary_late",    # a block boundary one 64-output group late
    "tail_dropped",     # the last 32 outputs of a window dropped
    "zero_history",     # zero history instead of the channelizer's
    "div_call",         # division by the call's outputs instead of the block's
    "shift_ignored",    # L_p ignored
    "source_0",         # the source index ignored: every source reads source 0
)
ROW_MUTANTS = ("zero_history", "shift_ignored", "source_0")      # the ones that change the virtual rows


def rows(wide, h, M, Q, incs, shifts, Ptab, m_first=0, n_out=None, mutant=None):
    """The virtual rows [n_sources, n_points, 2 n_out] uint8 of outputs [m_first, m_first + n_out): wide
    [n_sources, bytes] is every source's whole stream from sample 0 (what was run before the surveyed call, then the
    call); n_out None: to the end of the stream."""
    wide = np.asarray(wide, np.uint8).reshape(-1, np.asarray(wide).shape[-1])
    Q = max(1, int(Q))
    total = wide.shape[1] // 2 * Q // M
    n_out = total - m_first if n_out is None else n_out
    if mutant == "zero_history":
        wide = wide.copy()
        wide[:, :2 * (m_first * M // Q)] = 0x80               # (every call starts on a whole wide sample: M m_first / Q)
    if mutant == "shift_ignored":
        shifts = [0] * len(incs)
    out = np.empty((wide.shape[0], len(incs), 2 * n_out), np.uint8)
    for s in range(wide.shape[0]):
        src = wide[0] if mutant == "source_0" else wide[s]
        if Q == 1:
            for p, (d, L) in enumerate(zip(incs, shifts)):
                out[s, p] = cm.channel(src, h, M, int(d), int(L), Ptab, m_range=(m_first, m_first + n_out))
        else:
            out[s] = fm.channels(src, h, M, Q, [int(d) for d in incs], [int(L) for L in shifts], Ptab,
                                 m_range=(m_first, m_first + n_out))
    return out


def sample_magnitude(row_u8, mutant=None):
    """SignalDetector's per-sample magnitude of offset-binary byte pairs, int64 [.., n] from uint8 [.., 2 n]"""
    v = np.asarray(row_u8, np.int64) - 128
    a, b = np.abs(v[..., 0::2]), np.abs(v[..., 1::2])
    if mutant == "abs_127":
        a, b = np.minimum(a, 127), np.minimum(b, 127)
    if mutant == "mean_ab":
        return (a + b) >> 1
    return np.maximum(a, b) + (np.minimum(a, b) >> 1)


def reduce(rws, block_out, window=1024, oracle=None, mutant=None):
    """[n_sources, n_points, 2 n_out] rows -> [n_sources, n_blocks, n_points] uint32.  With an oracle and no defect in the
    detector, every entry is the oracle's block_magnitude of the block's signed bytes."""
    n_src, n_pts, nb = rws.shape
    n_out = nb // 2
    assert n_out % block_out == 0
    n_blocks = n_out // block_out
    out = np.empty((n_src, n_blocks, n_pts), np.uint32)
    if oracle is not None and mutant not in ("abs_127", "mean_ab", "boundary_late", "tail_dropped", "div_call"):
        s8 = (rws ^ 0x80).view(np.int8)
        for s in range(n_src):
            for p in range(n_pts):
                for b in range(n_blocks):
                    out[s, b, p] = oracle.block_magnitude(s8[s, p, 2 * b * block_out:2 * (b + 1) * block_out])
        return out
    mag = sample_magnitude(rws, mutant)                          # [n_src, n_pts, n_out]
    m = np.arange(n_out)
    if mutant == "tail_dropped":
        last = ((m % window) >= window - 32) | (m >= n_out - 32)
        mag = np.where(last, 0, mag)
    blk = m // block_out
    if mutant == "boundary_late":
        blk = np.maximum(m - 64, 0) // block_out
    for b in range(n_blocks):
        tot = mag[:, :, blk == b].sum(axis=2)
        out[:, b, :] = tot // (n_out if mutant == "div_call" else block_out)
    return out


def survey(wide, h, M, Q, incs, shifts, Ptab, block_out, m_first=0, n_out=None, window=1024, oracle=None, mutant=None):
    """magnitude[n_sources][n_blocks][n_points] of the call that gives outputs [m_first, m_first + n_out)."""
    r = rows(wide, h, M, Q, incs, shifts, Ptab, m_first, n_out, mutant if mutant in ROW_MUTANTS else None)
    return reduce(r, block_out, window, oracle, mutant)
