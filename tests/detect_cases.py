"""The inputs of the band activity detector's GPU test (tests/test_gpu_detect.py), built here so that the CPU tier can hold
the very same inputs to the mutation proof (tests/test_detect_host.py).  Everything is seeded; nothing here touches a GPU.
A case is one Detector object (a Cfg) and one call of [n_rows, N] uint32 powers.

The kernel gives a row to a wave, four rows to a workgroup, and walks the row 64 bins at a time, so the seams are the
multiples of 64 (a run that ends at, starts at, straddles or bridges one, an empty word between two hot ones) and the row
counts are 1, 3 (a workgroup partly used) and 65 (sixteen workgroups and one row)."""
import numpy as np

from tests import detect_model as dm

WORD = 64
RATE = 2048000
STATIONS = [  # offsets from the capture's centre, as tests/test_gpu_spectrum.py places them
    {"offset": -700e3, "kind": "fm", "amplitude": 25.0, "tone": 1000.0, "mode": "fm"},
    {"offset": 250e3, "kind": "am", "amplitude": 25.0, "tone": 700.0, "mode": "am"},
]
# the parameters of README's usage line: the upper median, 9 dB above it (8 x = 2048 / 256), the centre bin guarded, gaps of
# up to 8 bins bridged, at least 3 bins wide
def readme_cfg(N=1024, K=16):
    return dm.Cfg(N, N // 2, 2048, 1, 8, 3, K)


class Case:
    def __init__(self, name, cfg, power):
        self.name, self.cfg = name, cfg
        self.power = np.ascontiguousarray(power, np.uint32)
        assert self.power.ndim == 2 and self.power.shape[1] == cfg.n_bins
        dm.check_cfg(cfg)
        self.power.setflags(write=False)

    def __repr__(self):
        return self.name


NAMES = ["N64-flat", "N128-dup-rank", "N256-big", "N64-saturated", "N64-alternate-K4", "N2048-alternate", "N256-gaps-g0",
         "N256-gaps-g1", "N1024-gaps-g5", "N1024-gaps-g64", "N128-ends", "N2048-seams", "N1024-seams-K1", "N256-dc-d0",
         "N256-dc-d1", "N256-dc-d3", "N128-widths", "N64-peaks", "N128-random-65", "N1024-stations"]


def floor_row(rng, N, lo=90, hi=111):
    return rng.integers(lo, hi, N).astype(np.uint32)


def gaps_case(name, N, g, seed, K=None):
    """pairs of hot bins g apart (one run) and g + 1 apart (two), away from and across the seams, g = 0: neighbours"""
    rng = np.random.default_rng(seed)
    rows = np.stack([floor_row(rng, N) for _ in range(3)])
    for r, at0 in enumerate((3, WORD - 1 - g // 2, 2 * WORD - 1)):       # row 1: the gaps lie over a seam, row 2: start at one
        at = at0
        for gap in (g, g + 1, g, g + 1):
            if at + gap + 2 >= N:
                break
            rows[r, at] = 5000 + at
            rows[r, at + gap + 1] = 7000 + at
            at += gap + 1 + g + 9                                         # the next pair stands alone
    return Case(name, dm.Cfg(N, N // 2, 1024, 0, g, 1, K or N // 2), rows)


def dc_case(name, d):
    """the centre spike inside a run that bridges it (rows 0, 1: the run ends right at the guard's edge), alone (row 2)"""
    N, rng = 256, np.random.default_rng(700 + d)
    rows = np.stack([floor_row(rng, N) for _ in range(3)])
    rows[:, N // 2] = 4000000000
    rows[0, N // 2 - 6:N // 2 + 7] = rng.integers(3000, 9000, 13)
    rows[0, N // 2] = 4000000000
    rows[1, N // 2 - 9:N // 2 - 2] = rng.integers(3000, 9000, 7)          # ends at N / 2 - 3: the first bin d = 3 lets through
    rows[1, N // 2 + 3:N // 2 + 6] = rng.integers(3000, 9000, 3)
    rows[1, N // 2 - 1] = 2000                                            # hot unless guarded
    return Case(name, dm.Cfg(N, N // 2, 1024, d, 5, 2, 4), rows)


def cases(P):
    """P: the phasor table, [4096, 2] int16 (capi.channelizer_phasor_table()), for the rows of the two stations"""
    from rtlsdrdiags_amd import synth
    from tests import spectrum_model as sm
    out = []
    rng = np.random.default_rng(600)

    # all zero (f = 0 is raised to 1), one repeated value (nothing is above its own floor), 2^32 - 1 repeated; Q = 1.0
    flat = np.zeros((3, 64), np.uint32)
    flat[1], flat[2] = 7, dm.M32
    out.append(Case("N64-flat", dm.Cfg(64, 32, 256, 0, 0, 1, 32), flat))

    # long stretches of duplicates with the rank on their first, last and middle entry; values that differ in one byte only
    N = 128
    dup = np.zeros((5, N), np.uint32)
    for r, n_low in enumerate((N // 2, N // 2 - 9, N // 2 - 4)):         # 50 x n_low, 100 x 10, the rest far above
        dup[r] = rng.permutation(np.r_[np.full(n_low, 50), np.full(10, 100), np.full(N - n_low - 10, 3000 + 7 * r)])
    dup[3] = rng.permutation(np.r_[np.full(64, 0x01000000), np.full(8, 0x01000001), np.full(56, 0x7f000001)])
    dup[4] = rng.permutation(np.r_[np.full(63, 0x00ff00ff), np.full(2, 0x0100ff00), np.full(63, 0xff00ff00)])
    out.append(Case("N128-dup-rank", dm.Cfg(N, N // 2, 300, 0, 2, 1, 4), dup))

    # f Q passes 2^32 without reaching the saturation (f = 2^26 + .., Q = 2.0), hot bins up to 2^32 - 1: sums pass 2^32
    N = 256
    big = rng.integers(2 ** 26, 2 ** 26 + 1000, (3, N)).astype(np.uint32)
    big[0, 40:47] = dm.M32
    big[0, 60:70] = rng.integers(2 ** 31, 2 ** 32, 10)                    # over the seam at 64
    big[1, 250:256] = rng.integers(2 ** 30, 2 ** 32, 6)
    big[2, 0:3] = rng.integers(2 ** 28, 2 ** 29, 3)
    out.append(Case("N256-big", dm.Cfg(N, N // 2, 512, 0, 0, 2, 4), big))

    # the threshold saturates: nothing is hot, whatever stands in the row
    sat = rng.integers(2 ** 31, 2 ** 32, (1, 64)).astype(np.uint32)
    sat[0, 9] = dm.M32
    out.append(Case("N64-saturated", dm.Cfg(64, 32, 1024, 0, 0, 1, 1), sat))

    # every other bin hot at g = 0: N / 2 runs, more than K = 4 and exactly K = N / 2
    for name, N, K, n_rows in (("N64-alternate-K4", 64, 4, 1), ("N2048-alternate", 2048, 1024, 3)):
        alt = np.stack([floor_row(rng, N) for _ in range(n_rows)])
        alt[:, 1::2] = rng.integers(1000, 50000, (n_rows, N // 2))
        if n_rows > 1:
            alt[1] = np.roll(alt[1], 1)                                   # the hot bins on the even side: bin 0 starts a run
            alt[2, 1::2][::3] = 100                                       # holes: fewer runs than K, a zeroed tail
        out.append(Case(name, dm.Cfg(N, N // 2 - 1, 1024, 0, 0, 1, K), alt))

    out.append(gaps_case("N256-gaps-g0", 256, 0, 610))
    out.append(gaps_case("N256-gaps-g1", 256, 1, 611))
    out.append(gaps_case("N1024-gaps-g5", 1024, 5, 612, K=4))
    out.append(gaps_case("N1024-gaps-g64", 1024, 64, 613))

    # a run from bin 0 and a run to bin N - 1 in one row stay two (g = 5 would join them round the end)
    N = 128
    ends = np.stack([floor_row(rng, N) for _ in range(2)])
    ends[0, 0:3], ends[0, N - 3:N] = (900, 800, 700), (600, 700, 800)
    ends[1, 0], ends[1, N - 1] = 900, 900
    out.append(Case("N128-ends", dm.Cfg(N, N // 2, 1024, 0, 5, 1, 4), ends))

    # runs at every kind of seam: ending at 63, starting at 64, straddling 63 / 64, 255 / 256 and 1023 / 1024, spanning
    # three words, and two hot bins with one whole cold word between them (bridged at g = 64, a gap of 64)
    def seams(N, rng):
        rows = np.stack([floor_row(rng, N) for _ in range(3)])
        for a, b in ((57, 64), (128, 131), (250, 262), (1020, 1030), (N - 200, N - 30)):
            if b <= N:
                rows[0, a:b] = rng.integers(1000, 2 ** 20, b - a)
        for a, b in ((60, 68), (192, 256), (320, 321), (700, 1000)):
            if b <= N:
                rows[1, a:b] = rng.integers(1000, 2 ** 20, b - a)
        rows[1, 330:340:2] = 2000                                         # a run of gaps, bridged or not
        rows[2, [63, 128, 193, 258, 259, 400, 465]] = 3000                # 64 cold bins between: one run at g = 64
        return rows
    out.append(Case("N2048-seams", dm.Cfg(2048, 1024, 1024, 1, 64, 1, 4), seams(2048, np.random.default_rng(620))))
    out.append(Case("N1024-seams-K1", dm.Cfg(1024, 300, 1024, 0, 1, 2, 1), seams(1024, np.random.default_rng(621))))

    for d in (0, 1, 3):
        out.append(dc_case("N256-dc-d%d" % d, d))

    # widths of exactly m = 4 and of m - 1, solid and bridged (two hot bins three apart at g = 2: width 4, n_hot 2)
    N = 128
    wid = np.stack([floor_row(rng, N) for _ in range(1)])
    wid[0, 10:14] = (500, 600, 700, 800)
    wid[0, 30:33] = (500, 600, 700)
    wid[0, 62], wid[0, 65] = 900, 950
    wid[0, 90], wid[0, 92] = 900, 950
    wid[0, 100:104:3] = 1200
    out.append(Case("N128-widths", dm.Cfg(N, N // 2, 1024, 0, 2, 4, 4), wid))

    # equal peaks inside one run, next to each other and across a seam of a run that a second row starts at bin 0
    N = 64
    pk = np.stack([floor_row(rng, N) for _ in range(2)])
    pk[0, 20:30] = (700, 900, 800, 900, 600, 500, 900, 450, 460, 470)
    pk[1, 0:4] = (800, 800, 500, 800)
    pk[1, 60:64] = (500, 950, 950, 600)
    out.append(Case("N64-peaks", dm.Cfg(N, N // 2, 1024, 0, 0, 1, 4), pk))

    # 65 rows of noise with a heavy tail: runs wherever chance puts them
    N = 128
    rnd = (100 * np.exp(1.6 * np.random.default_rng(630).standard_normal((65, N)))).astype(np.uint32)
    out.append(Case("N128-random-65", dm.Cfg(N, N // 2, 768, 1, 1, 2, 4), rnd))

    # the two stations of synth.wideband, as the spectrum's model gives them: 2 blocks of 8 frames at N = 1024
    N, F, blocks = 1024, 8, 2
    u8 = synth.wideband(N * F * blocks, float(RATE), STATIONS, seed=31).reshape(1, -1)
    rows = sm.spectrum(u8, "u8", N, F, None, P)[0]
    out.append(Case("N1024-stations", readme_cfg(N), rows))

    assert [c.name for c in out] == NAMES
    return out
