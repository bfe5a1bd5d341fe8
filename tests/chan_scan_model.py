"""Model of scanner-driven wideband channels (include/iqdemod.h: iqd_channelizer_follow_scanner): per block, the
increment from the oracle chain's scanner frequency, the block cut by chan_model.channel (or silence out of band), then
the oracle chain's accept of that block - squelch, AGC and scanner step exactly as the reference's per-block order."""
import numpy as np

from tests import chan_model as cm


SCAN_MUTANTS = ("late", "oob_not_silence", "edge_in_band")   # wrong models, for the teeth tests


def tuning(M, centre_hz, station_hz, rotation=1, mutant=None):
    """The rule in Python integers: None out of band.  mutant "oob_not_silence": an out-of-band block is cut at the
    wrapped increment instead of being silence; "edge_in_band": the band edge o == Fs/2 is taken as in band."""
    fs = 256000 * M
    o = int(station_hz) + 64000 * int(rotation) - int(centre_hz)
    inside = -fs // 2 <= o <= fs // 2 if mutant == "edge_in_band" else -fs // 2 <= o < fs // 2
    if not inside and mutant != "oob_not_silence":
        return None
    return ((o << 32) + fs // 2) // fs % (1 << 32)


def scanner_hz(chain):
    return int(chain._lib.iqo_scanner_of(chain._h).contents.current_hz)


def follow(chain, wide_row, h, M, P, shift, centre_hz, block_out, n_blocks, m_first=0, rotation=1, late=False,
           mutant=None):
    """One following channel over n_blocks blocks of block_out outputs from output m_first (wide_row from sample 0).
    Returns (rows, pcm, magnitude, allowed, freq trace after each block).  late=True retunes one block late (a wrong
    model, for the teeth test), as does mutant="late"; the other mutants are tuning()'s."""
    late = late or mutant == "late"
    rows, pcm, mags, alw, trace = [], [], [], [], []
    inc_prev = None
    for b in range(n_blocks):
        inc = tuning(M, centre_hz, scanner_hz(chain), rotation, mutant)
        use = inc_prev if (late and b > 0) else inc
        inc_prev = inc
        m0 = m_first + b * block_out
        if use is None:
            blk = np.full(2 * block_out, 0x80, np.uint8)
        else:
            blk = cm.channel(wide_row, h, M, use, shift, P, m_range=(m0, m0 + block_out))
        p, mg, al = chain.accept_stream(blk, block_bytes=len(blk))
        rows.append(blk)
        pcm.append(p)
        mags.append(int(mg[0]))
        alw.append(int(al[0]))
        trace.append(scanner_hz(chain))
    return (np.concatenate(rows), np.concatenate(pcm) if pcm else np.zeros(0, np.int16), np.array(mags, np.uint32),
            np.array(alw, np.uint8), np.array(trace, np.uint64))
