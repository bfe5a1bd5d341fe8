"""Model of gain-following wideband channels (include/iqdemod.h: iqd_channelizer_follow_gain): per block, the gain in dB
from the oracle chain's IF gain, the block cut by chan_model.channel's stage a and rotation with the dB step in place of
the shift, then the oracle chain's accept of that block - squelch and AGC exactly in the reference's per-block order, so
that the next block's gain answers this block's magnitude."""
import numpy as np

from tests import chan_model as cm

M_J = (4096, 4598, 5161, 5793, 6502, 7298)        # lrint(4096 2^(j/6)): the header's IQD_GAIN_M0..5
G_MAX = 48

# wrong models, for the teeth tests
DEFECTS = ("late",            # the gain one block late
           "held",            # the gain of the call's first block held for the whole call
           "early",           # the gain taken after the same block's AGC step
           "m_trunc",         # m_j truncated instead of rounded
           "e_round",         # e rounded to nearest instead of g div 6
           "t_trunc",         # t truncated toward zero instead of floored
           "no_round",        # the rounding constant 2^(19-e) dropped
           "clamp46",         # clamp at 46 instead of 48
           "no_clamp",        # no clamp
           "sat127",          # sat8 at -127
           "manual_ignored",  # the manual gain ignored while the AGC is off (the default 24 instead)
           "ch0_gain")        # every channel using channel 0's gain


def mantissa(j, defect=None):
    return int(np.floor(4096 * 2 ** (j / 6))) if defect == "m_trunc" else M_J[j]


def rotated(wide_row, h, M, inc, P, m_range=None):
    """(rr, ri) int64 of outputs m_range: chan_model's stage a, then the rotation by P[(n d mod 2^32) >> 20]"""
    ar, ai = cm.channel(wide_row, h, M, inc, 0, P, m_range=m_range, stage_a=True)
    n_out = len(np.asarray(wide_row)) // 2 // M
    m0, m1 = (0, n_out) if m_range is None else m_range
    n = np.arange(m0, m1, dtype=np.int64) * M + M - 1
    idx = (((n.astype(np.uint64) * np.uint64(inc)) & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.int64)
    c, s = np.asarray(P, np.int64)[idx, 0], np.asarray(P, np.int64)[idx, 1]
    return ar * c + ai * s, ai * c - ar * s


def db_step(rr, ri, g, defect=None):
    """the last step: (rr, ri) -> interleaved offset-binary bytes at gain g dB"""
    g = int(g)
    g = g if defect == "no_clamp" else min(g, 46 if defect == "clamp46" else G_MAX)
    e, j = ((g + 3) // 6 if defect == "e_round" else g // 6), g % 6
    m = mantissa(j, defect)
    out = np.empty(2 * len(rr), np.uint8)
    for k, r in enumerate((rr, ri)):
        p = np.asarray(r, np.int64) * m
        t = np.sign(p) * (np.abs(p) >> 14) if defect == "t_trunc" else p >> 14
        rnd = 0 if defect == "no_round" else 1 << (19 - e)
        y = np.clip((t + rnd) >> (20 - e), -127 if defect == "sat127" else -128, 127)
        out[k::2] = (y + 128).astype(np.uint8)
    return out


def channel_db(wide_row, h, M, inc, g, P, m_range=None, defect=None):
    """One channel's output bytes at gain g dB: chan_model.channel(..., stage_a=True), the rotation, the dB step."""
    return db_step(*rotated(wide_row, h, M, inc, P, m_range), g, defect)


def follow(chain, wide_row, h, M, inc, P, block_out, n_blocks, m_first=0, defect=None, agc_on=True, gains0=None, rot=None):
    """One gain-following channel over the n_blocks blocks of block_out outputs of one call, from output m_first (wide_row
    from sample 0).  Returns (rows, pcm, magnitude, allowed, gain per block: the gain the block was cut with, before the
    clamp - the engine's gain-trace entry).  rot: rotated() of the whole row, computed once by the caller.  defect: one of
    DEFECTS; "ch0_gain" takes gains0, channel 0's gains of the same blocks; agc_on tells "manual_ignored" that the
    chain's AGC runs."""
    rows, pcm, mags, alw, gains = [], [], [], [], []
    g_prev = g_first = None
    for b in range(n_blocks):
        G = chain.rx_gain_db()
        use = G
        if defect == "late" and b > 0:
            use = g_prev
        elif defect == "held" and b > 0:
            use = g_first
        elif defect == "manual_ignored" and not agc_on:
            use = 24
        elif defect == "ch0_gain" and gains0 is not None:
            use = int(gains0[b])
        g_prev = G
        g_first = G if b == 0 else g_first
        m0 = m_first + b * block_out
        rr, ri = rotated(wide_row, h, M, inc, P, (m0, m0 + block_out)) if rot is None else (rot[0][m0:m0 + block_out],
                                                                                           rot[1][m0:m0 + block_out])
        blk = db_step(rr, ri, use, defect)
        p, mg, al = chain.accept_stream(blk, block_bytes=len(blk))
        if defect == "early":                      # (the chain has seen the right block; the rows show the wrong one)
            blk = db_step(rr, ri, chain.rx_gain_db(), defect)
        rows.append(blk)
        pcm.append(p)
        mags.append(int(mg[0]))
        alw.append(int(al[0]))
        gains.append(G)
    return (np.concatenate(rows), np.concatenate(pcm) if pcm else np.zeros(0, np.int16), np.array(mags, np.uint32),
            np.array(alw, np.uint8), np.array(gains, np.uint32))
