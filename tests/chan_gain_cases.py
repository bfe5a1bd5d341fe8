"""The inputs of tests/test_gpu_chan_gain.py (gain-following wideband channels), the smallest that reach every path of
chz_gain_kernel; tests/test_chan_gain_host.py proves on the numpy model (tests/chan_gain_model.py) that they expose the
model's defects.  Nothing here needs a GPU."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name M taps h n_src wide src inc shift follow bb calls agc manual threshold")
# taps: what the channelizer is created with (None: its default taps), h: the taps themselves; wide [n_src, bytes];
# follow [n_ch] bool: the channel follows its gain (the others are fixed, gain shift `shift`); bb: the engine's block_bytes;
# calls: row bytes per call (whole blocks, or one short block); agc: None (off), 0 (lowpass), 1 (Harris);
# manual: {call: {channel: gain in dB}} set before that call; threshold: the squelch's, for every channel

MANUAL = (0, 5, 6, 24, 47, 48, 60)                # the manual gains of the AGC-off cases, rotated over channels and calls
CARRIERS = ((0.146484375, 1.5), (-0.09765625, 6.0), (0.341796875, 100.0))   # (offset / Fs, amplitude in LSB): weak, medium,
#                                                                               near full scale; +300, -200, +700 kHz at M = 8


def inc_of(frac):
    """the increment of an offset given as a fraction of Fs"""
    return int(round(frac * 2 ** 32)) % 2 ** 32


def capture(M, n_samp, seed, sigma=0.5):
    from rtlsdrdiags_amd import synth
    fs = 256000 * M
    st = [{"offset": f * fs, "kind": "fm", "amplitude": a} for f, a in CARRIERS]
    return synth.wideband(n_samp, fs, st, seed=seed, sigma=sigma)


def k300_taps():
    """300 taps at M = 8 (10 K-chunks: more than stay in registers), a Hamming-windowed sinc of DC gain 32768"""
    x = np.arange(300) - 149.5
    w = np.sinc(2 * 0.06 * x) * np.hamming(300)
    h = np.rint(w / w.sum() * 32768).astype(np.int64)
    h[150] += 32768 - h.sum()
    return h.astype(np.int16)


def channel_plan(rng, n_follow, n_fixed, follow_sources, fixed_sources):
    """Following channels on the carriers in turn (a few hundred Hz apart so that no two rows agree), every fourth on a
    free frequency (noise only: its AGC runs to the rail); fixed channels at random increments with L = 0..8."""
    n = n_follow + n_fixed
    follow = np.zeros(n, bool)
    src, inc, shift = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    order = rng.permutation(n)                    # following and fixed channels interleaved
    for i, c in enumerate(order):
        if i < n_follow:
            follow[c] = True
            src[c] = follow_sources[i % len(follow_sources)]
            k = i // len(follow_sources)
            frac = 0.23 + 0.001 * k if k % 4 == 3 else CARRIERS[k % 4 % 3][0] + 0.0002 * (k // 4)
            inc[c] = inc_of(frac)
            shift[c] = 8 - i % 9                  # kept but ignored while the channel follows
        else:
            src[c] = fixed_sources[i % len(fixed_sources)]
            inc[c] = int(rng.integers(0, 2 ** 32))
            shift[c] = i % 9
    return src, inc, shift, follow


def manual_plan(n_ch, n_calls):
    return {k: {c: MANUAL[(c + k) % len(MANUAL)] for c in range(n_ch)} for k in range(n_calls)}


def cases(capi):
    out = []
    #     name              M  K     follow fixed src  follow on  fixed on  bb    blocks  agc   manual
    rows = (("M8-1ch-harris", 8, None, 1, 0, 1, [0], [0], 1024, 12, 1, False),
            ("M8-7ch-lowpass", 8, None, 7, 2, 1, [0], [0], 256, 12, 0, False),
            ("M2-9ch-harris", 2, None, 9, 3, 3, [0, 2], [1], 256, 12, 1, False),
            ("M7-65ch-harris", 7, None, 65, 4, 3, [0, 1, 2], [1], 1024, 12, 1, False),
            ("M8-7ch-off", 8, None, 7, 1, 1, [0], [0], 1024, 12, None, True),
            ("K300-9ch-off", 8, 300, 9, 2, 1, [0], [0], 256, 12, None, True),
            ("M8-2win-harris", 8, None, 9, 0, 1, [0], [0], 2560, 4, 1, False))
    for i, (name, M, K, nf, nx, n_src, fs_on, fx_on, bb, nblk, agc, man) in enumerate(rows):
        rng = np.random.default_rng(100 + i)
        taps = None if K is None else k300_taps()
        h = capi.channelizer_default_taps(M) if taps is None else taps
        calls = [nblk * bb] * 3 + [bb // 2]        # three calls of whole blocks, then one short block
        n_samp = sum(calls) // 2 * M
        wide = np.stack([capture(M, n_samp, 1000 * i + s) for s in range(n_src)])
        if name == "K300-9ch-off":                 # random bytes over the whole range, the rails among them
            wide = rng.integers(0, 256, wide.shape, dtype=np.uint8)
            wide[0, 64:72] = [0, 255, 255, 0, 0, 0, 255, 255]
        src, inc, shift, follow = channel_plan(rng, nf, nx, fs_on, fx_on)
        manual = manual_plan(nf + nx, len(calls)) if man else {}
        if name == "M8-7ch-lowpass":               # the operator moves a running AGC's gain between calls
            manual = {2: {int(np.nonzero(follow)[0][1]): 40}}
        out.append(Case(name, M, taps, h, n_src, wide, src, inc, shift, follow, bb, calls, agc, manual, -45))
    return out


def case_names():
    return ["M8-1ch-harris", "M8-7ch-lowpass", "M2-9ch-harris", "M7-65ch-harris", "M8-7ch-off", "K300-9ch-off", "M8-2win-harris"]


def chain_of(oracle, case, c):
    """the oracle chain of channel c as the engine of the GPU test is set up"""
    ch = oracle.chain()
    ch.set_mode("fm")
    ch.set_squelch(case.threshold)
    if case.agc is not None:
        ch.agc_set_type(case.agc)
        ch.agc_enable(True)
    return ch


def run_model(gm, oracle, case, P, c, defect=None, gains0=None, rot=None):
    """Channel c of a case through gm.follow, call by call: (rows, pcm, magnitude, allowed, gains), each a list per call."""
    ch = chain_of(oracle, case, c)
    s = int(case.src[c])
    out, m_at = [], 0
    for k, row in enumerate(case.calls):
        if c in case.manual.get(k, {}):
            ch.set_rx_gain_db(case.manual[k][c])
        bo = min(row, case.bb) // 2
        nb = row // 2 // bo
        g0 = None if gains0 is None else gains0[k]
        out.append(gm.follow(ch, case.wide[s], case.h, case.M, int(case.inc[c]), P, bo, nb, m_first=m_at, defect=defect,
                             agc_on=case.agc is not None, gains0=g0, rot=rot))
        m_at += row // 2
    ch.close()
    return [list(x) for x in zip(*out)]
