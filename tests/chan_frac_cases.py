"""The inputs of the fractional-rate channelizer's GPU test (tests/test_gpu_chan_frac.py), built here so that the CPU
tier can hold the very same inputs to the mutation proof (tests/test_chan_frac_host.py): a GPU test whose inputs cannot
see a defect proves nothing about it.  Everything is seeded; nothing here touches a GPU."""
import numpy as np

RATIOS = [(75, 8), (15, 2), (45, 4), (25, 2), (5, 2), (17, 8), (127, 2), (511, 8)]
INCS = [0, 1, 2 ** 31, 2 ** 31 - 1, 2 ** 32 - 1]
SUM_LIMIT = (2 ** 31 - 256) // 256            # per branch: 256 sum |h_r| <= 2^31 - 256


def stream(rng, n_bytes, kind):
    """random, or random with full-scale 0x00 / 0xFF / alternating stretches that drive both saturations"""
    u = rng.integers(0, 256, n_bytes, dtype=np.uint8)
    if kind == "rails":
        q = n_bytes // 4 // 2 * 2
        u[q:2 * q] = 0xFF
        u[2 * q:3 * q] = 0x00
        u[3 * q:4 * q] = np.tile(np.array([0, 0, 255, 255], np.uint8), q // 4 + 1)[:q]
    return u


def channel_set(rng, n_ch, n_src):
    src = np.arange(n_ch) % n_src
    rng.shuffle(src)
    inc = np.array([INCS[c] if c < len(INCS) else int(rng.integers(0, 2 ** 32)) for c in range(n_ch)], np.uint64)
    shift = np.array([(0, 8)[c % 2] if c < 12 else int(rng.integers(0, 9)) for c in range(n_ch)], np.uint8)
    return src.astype(np.uint32), inc, shift


def random_taps(rng, K, lim):
    h = rng.integers(-lim, lim + 1, K).astype(np.int16)
    h[0] = lim                                    # the byte split's extreme
    return h


def limit_taps(rng, K, Q):
    """every branch's sum |h_r| exactly at the limit, random signs"""
    h = np.zeros(K, np.int64)
    for r in range(Q):
        k = len(h[r::Q])
        v = np.full(k, SUM_LIMIT // k, np.int64)
        v[:SUM_LIMIT % k] += 1
        h[r::Q] = v * rng.choice([-1, 1], k)
    assert np.abs(h).max() <= 32639
    return h.astype(np.int16)


class Case:
    def __init__(self, capi, name, P, Q, taps, n_src, n_ch, seed, units=None, single_inc=None):
        rng = np.random.default_rng(seed)
        self.name, self.P, self.Q, self.n_src, self.n_ch = name, P, Q, n_src, n_ch
        if isinstance(taps, str) and taps == "default":
            self.taps, self.h = None, capi.channelizer_default_taps(P, Q)
        elif isinstance(taps, tuple) and taps[0] == "random":
            self.taps = self.h = random_taps(rng, taps[1], taps[2])
        else:
            self.taps = self.h = limit_taps(rng, taps[1], Q)
        self.unit = 64 * P                                       # the shortest call, bytes per source: 32 Q outputs
        self.units = max(3, 24 // Q) if units is None else units
        self.wide = np.stack([stream(rng, self.units * self.unit, "rails" if s % 2 == 0 else "random")
                              for s in range(n_src)])
        self.src, self.inc, self.shift = channel_set(rng, n_ch, n_src)
        if single_inc is not None:
            self.inc[:] = single_inc
        self.calls = [32 * Q * k for k in range(self.units)]     # the outputs at which the unit-sized calls begin

    def __repr__(self):
        return self.name


def cases(capi):
    out = []
    for i, (P, Q) in enumerate(RATIOS):                          # every ratio: default taps, two sources, seven channels
        out.append(Case(capi, "default-%d/%d" % (P, Q), P, Q, "default", 2, 7, 100 + i))
    out += [
        Case(capi, "K203-75/8", 75, 8, ("random", 203, 8000), 3, 64, 201),           # K not a multiple of Q
        Case(capi, "K3-17/8", 17, 8, ("random", 3, 32639), 1, 7, 202),               # K < Q: branches 3..7 empty
        Case(capi, "K1-5/2", 5, 2, ("random", 1, 32639), 2, 7, 203),                 # one tap: branch 1 empty
        Case(capi, "K8187-17/8", 17, 8, ("random", 8 * 1024 - 5, 8000), 1, 1, 204, single_inc=0x9e3779b9),   # ceil(K / Q) = 1024
        Case(capi, "K2047-5/2", 5, 2, ("random", 2047, 8000), 2, 7, 205),            # ceil(K / Q) = 1024, K odd
        Case(capi, "limit-45/4", 45, 4, ("limit", 4 * 300 - 1), 2, 7, 206),          # every branch's tap sum at the limit
        Case(capi, "limit-25/2", 25, 2, ("limit", 2 * 300 + 1), 1, 7, 207),
        Case(capi, "K33-5/2-300ch", 5, 2, ("random", 33, 32639), 3, 300, 208),       # several workgroups per source
        Case(capi, "default-75/8-64ch", 75, 8, "default", 3, 64, 209),               # several tiles per source
        Case(capi, "default-15/2-1ch", 15, 2, "default", 1, 1, 210, single_inc=12345678),
        Case(capi, "default-127/2-300ch", 127, 2, "default", 2, 300, 211, units=3),
    ]
    return out
