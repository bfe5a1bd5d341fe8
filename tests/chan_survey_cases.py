"""The inputs of the band survey's GPU test (tests/test_gpu_chan_survey.py), built here so that the CPU tier can hold the
very same inputs to the mutation proof (tests/test_chan_survey_host.py).  Everything is seeded; nothing here touches a
GPU.  A case is one channelizer, `pre` units run first (the history and sample count the survey must use), then one
surveyed call of `units` units (a unit: 64 M bytes per source, the shortest call)."""
import numpy as np

from tests import chan_frac_cases as fc

INCS = [0, 1, 2 ** 31, 2 ** 31 - 1, 2 ** 32 - 1]


def window(M, Q, K):
    """outputs per window of the kernels (iqd_chan_layout.h: ChzGeometry::t_max)"""
    kb = -(-K // Q)
    kp = -(-kb // 32) * 32
    if Q > 1:
        G = 16 * max(4, Q)
        return min(1024, (24576 // 2 - kp) * Q // M) // G * G
    return min(1024, (32768 // 2 - kp) // M) // 64 * 64


class Case:
    def __init__(self, capi, name, M, Q, taps, n_src, n_pts, block_bytes, units, pre, seed):
        rng = np.random.default_rng(seed)
        self.name, self.M, self.Q, self.n_src, self.n_pts = name, M, Q, n_src, n_pts
        self.block_bytes, self.block_out = block_bytes, block_bytes // 2
        if taps == "default":
            self.taps, self.h = None, capi.channelizer_default_taps(M, Q)
        else:
            self.taps = self.h = fc.random_taps(rng, taps[1], taps[2])
        self.unit = 64 * M                                       # bytes per source
        self.unit_out = 32 * Q                                   # outputs
        self.pre, self.units = pre, units
        self.m_first, self.n_out = pre * self.unit_out, units * self.unit_out
        assert self.n_out % self.block_out == 0 and self.n_out <= 8192
        self.window = window(M, Q, len(self.h))
        # random, and on the even sources full-scale rails, so that 0x00 (|-128|) and 0xFF occur in the virtual rows
        self.wide = np.stack([fc.stream(rng, (pre + units) * self.unit, "rails" if s % 2 == 0 else "random")
                              for s in range(n_src)])
        self.inc = np.array([INCS[p] if p < len(INCS) else int(rng.integers(0, 2 ** 32)) for p in range(n_pts)], np.uint64)
        self.shift = np.array([(8, 0)[p % 2] for p in range(n_pts)], np.uint8)     # L = 0 and 8 (one point: 8)

    @property
    def before(self):
        return self.wide[:, :self.pre * self.unit]

    @property
    def call(self):
        return self.wide[:, self.pre * self.unit:]

    def __repr__(self):
        return self.name


NAMES = ["M8-64", "M2-128", "M7-3win", "M8-K300-65pt", "M8-1pt-1blk", "5/2-256", "45/4-256", "75/8-65pt-3win", "75/8-tail"]


def cases(capi):
    out = [
        # block of 32 outputs: two blocks per 64-output group; the second window is 64 + 32 outputs
        Case(capi, "M8-64", 8, 1, "default", 3, 9, 64, 35, 2, 301),
        Case(capi, "M2-128", 2, 1, "default", 1, 7, 128, 34, 0, 302),
        # blocks of 2560 outputs: each spans three windows, the boundary lies inside one
        Case(capi, "M7-3win", 7, 1, "default", 3, 8, 5120, 160, 3, 303),
        # Kp = 320 > 256: the A operands from L2; 65 points: a second workgroup row
        Case(capi, "M8-K300-65pt", 8, 1, ("random", 300, 8000), 3, 65, 64, 35, 1, 304),
        Case(capi, "M8-1pt-1blk", 8, 1, "default", 1, 1, 16384, 256, 0, 305),
        Case(capi, "5/2-256", 5, 2, "default", 3, 9, 256, 18, 2, 306),
        Case(capi, "45/4-256", 45, 4, "default", 1, 7, 256, 9, 0, 307),
        Case(capi, "75/8-65pt-3win", 75, 8, "default", 3, 65, 5120, 20, 1, 308),
        Case(capi, "75/8-tail", 75, 8, "default", 1, 8, 256, 5, 3, 309),      # windows of 1024 and 256 outputs
    ]
    assert [c.name for c in out] == NAMES
    return out
