"""The inputs of tests/test_gpu_chan_fmt.py (the channelizer on signed captures), the smallest that reach every path of
chz_fmt_kernel; tests/test_chan_fmt_host.py proves on the numpy model that they expose every defect of
tests/chan_fmt_model.py.  Nothing here needs a GPU."""
import collections

import numpy as np

from tests import chan_fmt_model as fm

Case = collections.namedtuple("Case", "name fmt M taps h wide src inc shift n_src calls kind")
# taps: what the channelizer is created with (None: its default taps), h: the taps themselves; wide [n_src, 2 samples];
# calls: samples per call of the chained run (the long run is one call); kind: what the input was made for

EDGE_INCS = [0, 2 ** 31, 1, 2 ** 32 - 1]
LIMIT_SUM = 2 ** 23 - 1                                       # 256 sum |h| = 2^31 - 256


def window_outputs(M, K, fmt):
    """iqd_channelizer_window_outputs' formula: 2 B (t M + Kp) <= 32768, whole groups of 64, at most 1024"""
    kp = (K + 31) // 32 * 32
    return min(1024, (32768 // (2 * fm.RAIL_BYTES[fmt]) - kp) // M) // 64 * 64


def small_random(rng, n_samp, fmt):
    """Random input whose low bits matter: amplitude +-100 of 32768 for S16 (its 8-bit truncation is silence: the high
    byte is 0 or -1), +-100 for S8, with the rails' extremes once each."""
    w = rng.integers(-100, 101, 2 * n_samp).astype(fm.DTYPE[fmt])
    info = np.iinfo(fm.DTYPE[fmt])
    w[6:10] = [info.min, info.max, info.max, info.min]
    return w


def full_random(rng, n_samp, fmt):
    info = np.iinfo(fm.DTYPE[fmt])
    return rng.integers(info.min, info.max + 1, 2 * n_samp).astype(fm.DTYPE[fmt])


def channel_set(rng, n_ch, sources):
    """n_ch channels spread over `sources` (a list; a source not in it gets none): the edge increments first, random ones
    after; L = 0 and 8 among the shifts"""
    src = np.array([sources[c % len(sources)] for c in range(n_ch)], np.uint32)
    inc = rng.integers(0, 2 ** 32, n_ch, dtype=np.uint64)
    inc[:min(n_ch, 4)] = EDGE_INCS[:min(n_ch, 4)]
    shift = rng.integers(0, 9, n_ch).astype(np.uint8)
    shift[0] = 8
    if n_ch > 1:
        shift[1] = 0
    return src, inc, shift


def chain_calls(M, K, n_out):
    """samples per call: ceil(Kp / (32 M)) + 2 calls of the shortest length (32 outputs), so that a sample is carried
    through the history across every one of them, then the rest as one call"""
    kp = (K + 31) // 32 * 32
    chain = -(-kp // (32 * M)) + 2
    assert n_out > 32 * chain
    return [32 * M] * chain + [(n_out - 32 * chain) * M]


def plant_half(row, h, M, P, m_star):
    """Changes one sample of the row so that channel 0's (increment 0: real taps) Ar of output m_star is exactly 2^15 mod
    2^16 (S8: 128 mod 256) - the point where stage a's rounding constant decides.  The tap with the fewest factors of 2 serves: an
    odd one is invertible mod 2^16."""
    from tests import chan_model as cm
    gr = cm.channel_taps(h, 0, P)[0]
    n = m_star * M + M - 1
    ks = np.arange(min(len(gr), n + 1))
    v2 = [(int(g) & -int(g)) if g else 1 << 20 for g in gr[ks]]   # the power of 2 in each tap
    k0 = int(np.argmin(v2))
    p2 = v2[k0]
    xr = row[0::2].astype(np.int64)
    rest = int((gr[ks] * xr[n - ks]).sum()) - int(gr[k0]) * int(xr[n - k0])
    mod = 2 ** (8 * row.dtype.itemsize)                       # (x mod `mod` is a sample value; A is wanted mod `mod` too)
    T = (mod // 2 - rest) % mod                               # gr[k0] v = T (mod 2^16)
    assert T % p2 == 0, "no sample value puts this output on the half point"
    v = (T // p2 * pow(int(gr[k0]) // p2, -1, mod // p2)) % (mod // p2)
    v = (v + mod // 2) % mod - mod // 2
    assert (rest + int(gr[k0]) * v) % mod == mod // 2
    row[2 * (n - k0)] = v
    row[2 * (n - k0) + 1] = 0                                 # (gi = 0: Q does not enter Ar; keep it quiet)


def limit_taps():
    """K = 1024 taps exactly at sum |h| = 2^23 - 1.  All but two sit at k = 1 mod 4 with the sign alternating, so that for
    an increment of an odd multiple of 2^29 (k x 45 degrees) every one of those complex taps lies on the same diagonal:
    sum(|gr| + |gi|) = 1.414 sum |h|, the largest there is."""
    h = np.zeros(1024, np.int64)
    k = np.arange(1, 1024, 4)
    h[k] = np.where(k % 8 == 1, 32639, -32639)
    h[3], h[7] = 32639, LIMIT_SUM - 257 * 32639
    assert np.abs(h).sum() == LIMIT_SUM and np.abs(h).max() == 32639
    return h.astype(np.int16)


def limit_case(P, fmt):
    """M = 8, five sources with one channel each: 0 degrees and the four diagonals.  A source is four segments of 2048
    samples, the input sign-matched to its channel's taps (every output sees the same alignment: the taps' pattern has
    period 8 = M) for (rail, extreme) = (re, max), (re, min), (im, max), (im, min): in the second half of a segment |A| is
    the largest the taps allow, Lo leaves int32 and sat16 is reached on that rail at that end."""
    from tests import chan_model as cm
    h = limit_taps()
    M, seg = 8, 2048
    incs = [0, 2 ** 29, 3 * 2 ** 29, 5 * 2 ** 29, 7 * 2 ** 29]
    info = np.iinfo(fm.DTYPE[fmt])
    wide = np.zeros((len(incs), 2 * 4 * seg), fm.DTYPE[fmt])
    for s, d in enumerate(incs):
        gr, gi = cm.channel_taps(h, d, P)
        for q, (rail, top) in enumerate([(0, True), (0, False), (1, True), (1, False)]):
            nn = np.arange(q * seg, (q + 1) * seg)
            k = (M - 1 - nn) % 8                             # x[n] meets g[k] with k = (n_m - n) mod 8, n_m = M - 1 mod 8
            # the sign pattern of the taps over one period (k and k + 8 j agree in sign wherever both are non-zero)
            sr = np.array([np.sign(gr[kk::8].sum()) for kk in range(8)])[k]
            si = np.array([np.sign(gi[kk::8].sum()) for kk in range(8)])[k]
            wr, wi = (sr, -si) if rail == 0 else (si, sr)    # Ar = sum gr xr - gi xi, Ai = sum gr xi + gi xr
            if not top:
                wr, wi = -wr, -wi
            wide[s, 2 * nn] = np.where(wr > 0, info.max, info.min)
            wide[s, 2 * nn + 1] = np.where(wi > 0, info.max, info.min)
    n = len(incs)
    return Case("limit-" + fmt, fmt, M, h, h, wide, np.arange(n, dtype=np.uint32), np.array(incs, np.uint64),
                np.array([0, 8, 0, 3, 8], np.uint8), n, chain_calls(M, len(h), 4 * seg // M), "limit")


def cases(capi):
    P = capi.channelizer_phasor_table()
    out = []
    for fmt in ("s16", "s8"):
        rng = np.random.default_rng(7 if fmt == "s16" else 8)
        # (M, channels, sources, those with channels, windows of the long call): default taps, small random input
        for M, n_ch, n_src, used, nwin in ((2, 9, 3, [0, 2], 2), (7, 7, 1, [0], 1), (8, 65, 1, [0], 2), (64, 1, 1, [0], 3)):
            h = capi.channelizer_default_taps(M)
            t = window_outputs(M, len(h), fmt)
            n_out = nwin * t + 32                            # whole windows and a 32-output tail
            wide = np.stack([small_random(rng, n_out * M, fmt) for _ in range(n_src)])
            src, inc, shift = channel_set(rng, n_ch, used)
            plant_half(wide[0], h, M, P, n_out - 7)
            out.append(Case("M%d-%dch-%s" % (M, n_ch, fmt), fmt, M, None, h, wide, src, inc, shift, n_src,
                            chain_calls(M, len(h), n_out), "small"))
        # K = 1; K = 300 at M = 8: more K-chunks than stay in registers, the A operands read per group
        # (small taps: full-scale input stays inside the output's range at the middle gains)
        for name, M, h, n_ch in (("K1", 8, np.array([129], np.int16), 2),
                                 ("K300", 8, rng.integers(-30, 31, 300).astype(np.int16), 9)):
            n_out = 192
            wide = full_random(rng, n_out * M, fmt)[None]
            src, inc, shift = channel_set(rng, n_ch, [0])
            shift[:] = [7, 8] + [0, 6, 5][:n_ch - 2] + [4] * max(0, n_ch - 5)
            plant_half(wide[0], h, M, P, n_out - 7)
            out.append(Case("%s-%s" % (name, fmt), fmt, M, h, h, wide, src, inc, shift, 1, chain_calls(M, len(h), n_out), "tiny"))
        out.append(limit_case(P, fmt))
    return out


def case_names():
    return ["%s-%s" % (n, fmt) for fmt in ("s16", "s8")
            for n in ("M2-9ch", "M7-7ch", "M8-65ch", "M64-1ch", "K1", "K300", "limit")]
