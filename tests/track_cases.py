"""The inputs of the band activity tracker's GPU test (tests/test_gpu_track.py), built here so that the CPU tier can hold the
very same inputs to the mutation proof (tests/test_track_host.py).  Everything is seeded; nothing here touches a GPU.

A case is one Tracker object (a Cfg) and a script of calls: ("run", b0, b1) hands blocks b0 .. b1 - 1 of the case's detector
arrays to one call, ("reset",) is iqd_track_reset.  The detector arrays are written by hand - a list of (first_bin,
last_bin, peak_power, centroid_q8) per (source, block) - at the smallest shapes that can go wrong; what lies past a row's
n_found is seeded garbage unless the case says otherwise.

The kernel gives a source to a wave and a slot to a lane, and fetches 64 records per trip, so the seams are S = 1 and 64,
K = 64 / 65 and up, and more than one source."""
import numpy as np

from tests import detect_cases as dc
from tests import detect_model as dm
from tests import track_model as tm

RATE = dc.RATE
STATIONS = dc.STATIONS


class Case:
    def __init__(self, name, cfg, dets, n_blocks, calls=None, n_found=None, garbage=True, seed=0):
        """dets: {(source, block): [(first, last, peak, centroid), ...]}; n_found: {(source, block): value} where it is
        not the list's length (the list then holds the K records the row really has)"""
        tm.check_cfg(cfg)
        self.name, self.cfg, self.n_blocks = name, cfg, n_blocks
        self.calls = calls or [("run", 0, n_blocks)]
        K, N = cfg.max_detections, cfg.n_bins
        rng = np.random.default_rng(1000 + seed)
        raw = rng.integers(0, 256, (cfg.n_sources, n_blocks, K, 32), dtype=np.uint8) if garbage else \
            np.zeros((cfg.n_sources, n_blocks, K, 32), np.uint8)
        self.det = np.ascontiguousarray(raw).view(dm.DET_DTYPE).reshape(cfg.n_sources, n_blocks, K)
        self.rows = np.zeros((cfg.n_sources, n_blocks), dm.ROW_DTYPE)
        self.rows["floor"], self.rows["threshold"] = 100, 800
        for (j, b), lst in dets.items():
            assert len(lst) <= K and lst == sorted(lst, key=lambda r: r[0])
            for i, (first, last, peak, cq) in enumerate(lst):
                assert 0 <= first <= last < N and 256 * first <= cq < 256 * (last + 1) and 0 < peak <= tm.M32
                self.det[j, b, i] = (first, last, (first + last) // 2, peak, peak * (last - first + 1), cq, last - first + 1)
            self.rows[j, b]["n_found"] = len(lst)
            self.rows[j, b]["n_hot_bins"] = sum(r[1] - r[0] + 1 for r in lst)
        for (j, b), v in (n_found or {}).items():
            self.rows[j, b]["n_found"] = v
        self.rows.setflags(write=False)
        self.det.setflags(write=False)

    def __repr__(self):
        return self.name


def run_script(case, tracker):
    """the case's calls on a tracker with run(rows, det) and reset(): (slots, blocks) of all the blocks, in order"""
    slots, blocks = [], []
    for op in case.calls:
        if op[0] == "reset":
            tracker.reset()
        else:
            s, b = tracker.run(np.ascontiguousarray(case.rows[:, op[1]:op[2]]), np.ascontiguousarray(case.det[:, op[1]:op[2]]))
            slots.append(s)
            blocks.append(b)
    return np.concatenate(slots, axis=1), np.concatenate(blocks, axis=1)


def model(case, defects=()):
    return run_script(case, tm.Tracker(case.cfg, defects))


NAMES = ["N64-S3-life", "N64-S3-split-reset", "N64-ties", "N64-gate", "N64-nearest", "N64-full-S1", "N64-full-S3",
         "N64-close-and-arrive", "N64-B0-H1", "N64-A1", "N64-A256", "N64-found-over-K1", "N64-found-over-K4", "N2048-K128-S64",
         "N2048-edges-bias", "N64-sources3", "N64-hits-300", "N64-widths", "N256-chained"]


def d(bin_, q8=0, width=3, peak=5000):
    """a detection centred q8 / 256 of a bin above bin_'s lower edge, `width` bins wide"""
    first = max(bin_ - (width - 1) // 2, 0)
    return (first, first + width - 1, peak, 256 * bin_ + q8)


def cfg(n_sources=1, N=64, K=4, S=3, G=512, H=3, B=2, A=64, bias=0, edges=None):
    return tm.Cfg(n_sources, N, K, S, G, H, B, A, bias, tuple(edges or (max(N // 64, 1) + 1, N // 16, N // 4)))


def chained_wide():
    """The chained case's capture: synth.wideband at N = 256, F = 8, 24 blocks, seed 31; the FM station at -700 kHz always on,
    the AM station at +250 kHz keyed on over samples [6.5 N F, 14.3 N F).  [1, bytes] uint8."""
    from rtlsdrdiags_amd import synth
    N, F, blocks = 256, 8, 24
    stations = [STATIONS[0], dict(STATIONS[1], on=[(6.5 * N * F, 14.3 * N * F)])]
    return np.ascontiguousarray(synth.wideband(N * F * blocks, float(RATE), stations, seed=31)).reshape(1, -1)


CHAINED = dict(N=256, F=8, blocks=24, S=4, G=512, H=3, B=2, A=64)


def chained_cfg():
    c = CHAINED
    return cfg(1, c["N"], 16, c["S"], c["G"], c["H"], c["B"], c["A"])


def cases(P):
    """P: the phasor table, [4096, 2] int16 (capi.channelizer_phasor_table()), for the chained case's spectrum rows"""
    from tests import spectrum_model as sm
    out = []

    # a life: a track drifts up and down (differences of both signs through the shift), opens at its third hit, fades for
    # one and two blocks (held), then for three (closed in the third, zeroed in the fourth); a second one is seen once
    # (tentative, dropped at its first miss) and later twice in a row then lost; a third comes back where the first closed
    life = {}
    drift = [0, 37, 75, 30, -60, -130, -20, 90]
    for b, q in enumerate(drift):
        life[(0, b)] = [d(20, 100 + q)]
    life[(0, 2)] = [d(20, 100 + drift[2]), d(40, 10)]                    # 40: one hit only
    life[(0, 8)] = []                                                    # one miss
    life[(0, 9)] = [d(20, 140)]
    life[(0, 10)], life[(0, 11)] = [], []                                # two misses: still held
    life[(0, 12)] = [d(20, 90), d(50, 0, width=5)]
    life[(0, 13)] = [d(50, 30, width=7)]                                 # 20 starts to miss; 50 has two hits
    life[(0, 14)], life[(0, 15)] = [], []                                # 50 dropped at 14; 20 closes at 15
    life[(0, 16)] = [d(20, 90)]                                          # a new id in the slot the closed record left
    life[(0, 17)] = [d(20, 80), d(21, 200)]                              # the second one is within the gate of the same slot
    out.append(Case("N64-S3-life", cfg(), life, 18, seed=1))
    # the same blocks in three calls, a reset and two more calls: state and next_id are carried, and cleared by the reset
    out.append(Case("N64-S3-split-reset", cfg(), life, 18, seed=2,
                    calls=[("run", 0, 1), ("run", 1, 7), ("run", 7, 12), ("reset",), ("run", 12, 14), ("run", 14, 18)]))

    # two slots equally far from one detection (the lowest slot), two detections equally far from one slot (the first
    # detection; the second becomes a new track); A = 256, so centres are exactly where the detections were
    ties = {(0, 0): [d(10), d(14)],                                      # slots 0, 1 at 2560, 3584
            (0, 1): [d(12)],                                             # 3072: 512 from both -> slot 0; slot 1 misses
            (0, 2): [d(10), d(14)],                                      # slot 0 (now at 3072) is 512 from both: detection 0
            (0, 3): [d(12)]}                                             # slot 0 at 2560 and the new slot 2 at 3584: slot 0
    out.append(Case("N64-ties", cfg(G=512, H=1, B=1, A=256), ties, 4, seed=3))

    # a distance of exactly G (matched) and of G + 1 (a new track)
    gate = {(0, 0): [d(30, 0)], (0, 1): [d(32, 0)], (0, 2): [d(30, 0)], (0, 3): [d(31, 255, width=2)], (0, 4): [d(30, 0)],
            (0, 5): [d(27, 255)]}
    out.append(Case("N64-gate", cfg(G=512, H=2, B=0, A=256), gate, 6, seed=4))
    # G = 511 on the same blocks: 512 is now G + 1
    # the nearest slot is not the first one in the gate; the gate is wide
    near = {(0, 0): [d(10), d(20)], (0, 1): [d(18)], (0, 2): [d(11), d(19)], (0, 3): [d(16, 128)]}
    out.append(Case("N64-nearest", cfg(G=2560, H=1, B=3, A=128), near, 4, seed=5))

    # every slot full and one detection more, S = 1 and S = 3; K = 1 at S = 1
    out.append(Case("N64-full-S1", cfg(K=4, S=1, H=2, B=1), {(0, 0): [d(8), d(30)], (0, 1): [d(8), d(30), d(50)],
                                                             (0, 2): [d(30), d(50)], (0, 3): [d(50)], (0, 4): [d(50)]}, 5, seed=6))
    out.append(Case("N64-full-S3", cfg(K=4, S=3, H=2, B=1), {(0, 0): [d(8), d(20), d(30), d(50)], (0, 1): [d(8), d(20), d(30), d(50)],
                                                             (0, 2): [d(20), d(50)], (0, 3): [d(20), d(40), d(50)],
                                                             (0, 4): [d(20), d(40), d(50), d(60)]}, 5, seed=7))

    # a track closes, a tentative one is dropped, and a new detection arrives in the same block with no other slot free:
    # it is unplaced in that block and placed in the next
    ca = {(0, 0): [d(10), d(30)], (0, 1): [d(10), d(30)], (0, 2): [d(10), d(50)],     # 30 misses once; 50 is unplaced (S = 2)
          (0, 3): [d(10), d(50)],                                                     # 30 closes (B = 1); 50 unplaced again
          (0, 4): [d(10), d(50)],                                                     # 50 takes the zeroed slot
          (0, 5): [d(10), d(20)],                                                     # 50 (tentative) dropped; 20 unplaced
          (0, 6): [d(10), d(20)]}
    out.append(Case("N64-close-and-arrive", cfg(S=2, H=2, B=1), ca, 7, seed=8))

    # B = 0 and H = 1: open on allocation, close at the first miss
    out.append(Case("N64-B0-H1", cfg(S=3, H=1, B=0, A=64), {(0, 0): [d(10)], (0, 1): [d(10, 40), d(40)], (0, 2): [d(40)],
                                                            (0, 3): [d(10), d(40)], (0, 4): [], (0, 5): []}, 6, seed=9))
    # A = 1: a difference of -1 .. -255 moves the centre by -1 (the floor), +1 .. +255 not at all; A = 256: it follows
    a1 = {(0, b): [d(20, q)] for b, q in enumerate([128, 127, 0, 255, 200, 1, 128 + 256, 0])}
    out.append(Case("N64-A1", cfg(G=1024, H=2, A=1), a1, 8, seed=10))
    out.append(Case("N64-A256", cfg(G=1024, H=2, A=256), a1, 8, seed=11))

    # n_found above K: only K records exist, and the next row's records must not be taken for this row's
    over = {(0, 0): [d(10)], (0, 1): [d(10)], (0, 2): [d(30)], (0, 3): [d(10)]}
    out.append(Case("N64-found-over-K1", cfg(K=1, S=3, H=2, B=2), over, 4, n_found={(0, 0): 3, (0, 1): 2, (0, 3): 40}, seed=12))
    over4 = {(0, 0): [d(5), d(15), d(25), d(35)], (0, 1): [d(45), d(55)], (0, 2): [d(5), d(15), d(25), d(35)], (0, 3): []}
    out.append(Case("N64-found-over-K4", cfg(K=4, S=8, H=2, B=2), over4, 4, n_found={(0, 0): 6, (0, 2): 2 ** 32 - 1}, seed=13))

    # N = 2048, K = 128, S = 64: 64 tracks from 64 detections, then 100 detections of which records 36 .. 99 - over the
    # 64-record seam of the fetch - are the tracks' and records 0 .. 35 find no slot; then 70 with every second track missing
    pos = [40 + 20 * i for i in range(100)]
    big = {(0, 0): [d(p, 17, peak=1000 + p) for p in pos[36:]],
           (0, 1): [d(p, 60, width=5, peak=2000 + p) for p in pos],
           (0, 2): [d(p, 200, peak=3000 + p) for p in pos[:30] + pos[36::2] + [2040]],
           (0, 3): [d(p, 90, peak=3000 + p) for p in pos[30:]]}
    out.append(Case("N2048-K128-S64", cfg(N=2048, K=128, S=64, G=300, H=2, B=0, A=200, edges=(4, 5, 2049)), big, 4, seed=14))

    # centroids at 0, just below and above 128 N and at 256 N - 1, at both ends of the shift, with a bias that wraps
    for N, name in ((2048, "N2048-edges-bias"),):                     # (N = 64 has centroids on both sides of the centre in every other case)
        e = {(0, 0): [(0, 0, 900, 0), d(N // 2 - 1, 255), d(N // 2, 0), (N - 1, N - 1, 900, 256 * N - 1)],
             (1, 0): [(0, 2, 900, 1), d(N // 2 - 2, 3), d(N // 2, 1), (N - 3, N - 1, 900, 256 * N - 2)]}
        for j in range(2):
            e[(j, 1)] = e[(j, 0)]
        out.append(Case(name, cfg(2, N, 4, 4, G=0, H=1, A=256, bias=0xC0000001), e, 2, seed=15))

    # three sources with different histories: ids count per source
    src3 = {}
    for j in range(3):
        for b in range(5):
            src3[(j, b)] = [d(10 + 7 * j + 13 * k, 30 * b) for k in range(1 + (j + b) % 3)]
    out.append(Case("N64-sources3", cfg(3, 64, 4, 3, H=2, B=1), src3, 5, calls=[("run", 0, 2), ("run", 2, 5)], seed=16))

    # 300 blocks of one detection: hits stops at 255, age does not
    out.append(Case("N64-hits-300", cfg(K=1, S=1, H=255, B=0), {(0, b): [d(33, b % 50)] for b in range(300)}, 300, seed=17))

    # the class is the widest the track has been, not the last width; widths at and one under every edge
    wid = {(0, b): [d(32, 0, width=w)] for b, w in enumerate([1, 2, 4, 3, 8, 7, 15, 16, 2])}
    out.append(Case("N64-widths", cfg(K=1, S=2, G=1024, H=1, edges=(2, 8, 16)), wid, 9, seed=18))

    # the chained case: the detector's model on the spectrum's model of the keyed capture (zeros past n_found, as the
    # detector writes them)
    c = CHAINED
    power = sm.spectrum(chained_wide(), "u8", c["N"], c["F"], None, P)[0]
    rows, det = dm.detect(power, dc.readme_cfg(c["N"]))
    ch = Case("N256-chained", chained_cfg(), {}, c["blocks"], garbage=False, seed=19)
    ch.rows, ch.det = rows.reshape(1, -1), det.reshape(1, c["blocks"], 16)
    out.append(ch)

    assert [x.name for x in out] == NAMES
    return out
