"""The inputs of the band track measurements' GPU test (tests/test_gpu_measure.py), built here so that the CPU tier can hold
the very same inputs to the mutation proof (tests/test_measure_host.py).  Everything is seeded; nothing here touches a GPU.

A case is one Measure object (a Cfg) and its three input arrays, written by hand at the smallest shapes that can go wrong.
Of a detector row only the floor means anything and of a slot only track_id, state, first_bin and last_bin; every other byte
of both is seeded garbage, which the kernel must not look at.

The kernel gives a (source, block) to a workgroup of four waves, max(N / 256, 1) consecutive bins to a thread (scalar loads
up to N = 512, 16-byte loads from N = 1024), slot s to wave s mod 4, and searches a window in stretches of ceil(span / 64)
bins: so the seams are N = 64 (one wave's lanes), 256, 512, 1024, 2048; S = 1, 4 / 5, 64; spans of 1, 64, 65, 128, 129, N."""
import numpy as np

from tests import detect_cases as dc
from tests import detect_model as dm
from tests import measure_model as mm
from tests import track_model as tm

RATE = dc.RATE
M32 = 2 ** 32 - 1
FREE, CLOSING, TENTATIVE, ACTIVE = "free", "closing", 1, 2


class Case:
    def __init__(self, name, cfg, power, floors, slots, seed=0):
        """power [J, B, N]; floors [J, B] or one number; slots: {(source, block, slot): (kind, first, last)}, kind FREE, CLOSING,
        TENTATIVE or ACTIVE - slots not named are free"""
        mm.check_cfg(cfg)
        self.name, self.cfg = name, cfg
        J, N, S = cfg.n_sources, cfg.n_bins, cfg.n_slots
        self.power = np.ascontiguousarray(power, np.uint32).reshape(J, -1, N)
        B = self.n_blocks = self.power.shape[1]
        rng = np.random.default_rng(2000 + seed)
        self.rows = np.ascontiguousarray(rng.integers(0, 256, (J, B, 16), dtype=np.uint8)).view(dm.ROW_DTYPE).reshape(J, B)
        self.rows["floor"] = np.broadcast_to(np.asarray(floors, np.uint32), (J, B))
        self.slots = np.ascontiguousarray(rng.integers(0, 256, (J, B, S, 32), dtype=np.uint8)).view(tm.SLOT_DTYPE).reshape(J, B, S)
        self.slots["track_id"] = 0
        self.slots["state"] = 0
        next_id = 0
        for (j, b, s), (kind, first, last) in slots.items():
            assert 0 <= first <= last < N
            next_id += 1
            self.slots["track_id"][j, b, s] = 0 if kind == FREE else next_id + 1000 * j
            self.slots["state"][j, b, s] = 0 if kind in (FREE, CLOSING) else kind
            self.slots["first_bin"][j, b, s], self.slots["last_bin"][j, b, s] = first, last
        for a in (self.power, self.rows, self.slots):
            a.setflags(write=False)

    def __repr__(self):
        return self.name


def model(case, defects=()):
    return mm.measure(case.power, case.rows, case.slots, case.cfg, defects)


def cfg(J=1, N=64, S=1, d=1, m=2, beta=328, c=1, min_sum=0, cq8=128, wide=16):
    return mm.Cfg(J, N, S, d, m, beta, c, min_sum, cq8, wide)


def noise(rng, shape, lo=90, hi=111):
    """around a floor of 100: bins under it, at it and over it"""
    return rng.integers(lo, hi, shape).astype(np.uint64)


def bump(p, centre, half, top):
    """a triangle of height `top` over centre - half .. centre + half, added in place (clipped to the row)"""
    N = p.shape[-1]
    for k in range(max(centre - half, 0), min(centre + half, N - 1) + 1):
        p[..., k] += top * (half + 1 - abs(k - centre)) // (half + 1)


NAMES = ["N64-S1-basics", "N64-edges", "N64-guard", "N64-single-bin", "N64-states-overlap", "N64-empty", "N64-saturated",
         "N2048-saturated", "N64-peak-ties", "N64-beta0", "N64-beta-max", "N64-carrier-c0", "N64-carrier-c8-edge", "N64-minsum",
         "N64-obw-edge", "N64-hints", "N128-sources3", "N256-random", "N512-random", "N1024-random", "N2048-S64"]


def random_case(name, N, J, B, S, seed, **kw):
    """noise with a few stations of every size, floors that differ from source to source, slots of every kind over windows of
    the spans where the search changes its stretch"""
    rng = np.random.default_rng(seed)
    p = noise(rng, (J, B, N))
    for j in range(J):
        for b in range(B):
            for _ in range(6):
                bump(p[j, b], int(rng.integers(0, N)), int(rng.choice([0, 1, 3, 9, 40])), int(rng.choice([30, 4000, 10 ** 6, 2 ** 31])))
    p = np.minimum(p, M32)
    spans = [1, 2, 3, 10, 63, 64, 65, 128, 129, N // 2, N]
    slots = {}
    for j in range(J):
        for b in range(B):
            for s in range(S):
                span = min(int(rng.choice(spans)), N)
                first = int(rng.integers(0, N - span + 1))
                if s % 16 == 3:                                       # the row's ends
                    first = 0 if b % 2 else N - span
                kind = [ACTIVE, ACTIVE, TENTATIVE, FREE, CLOSING][int(rng.integers(0, 5))]
                slots[(j, b, s)] = (kind, first, first + span - 1)
    floors = np.array([[100 + 7 * j + (b % 2) for b in range(B)] for j in range(J)])
    return Case(name, cfg(J, N, S, **kw), p, floors, slots, seed)


def cases():
    out = []
    rng = np.random.default_rng(77)

    # one slot, three blocks with different power: a station inside its window, noise around it with bins under, at and over
    # the floor; the run sits off the window's centre so that a centroid counted from lo is another number
    p = noise(rng, (1, 3, 64))
    for b in range(3):
        bump(p[0, b], 20 + 3 * b, 3, 5000 * (b + 1))
        p[0, b, 14] = 100                                             # at the floor, inside every window
    sl = {(0, b, 0): (ACTIVE, 16 + 3 * b, 24 + 3 * b) for b in range(3)}
    out.append(Case("N64-S1-basics", cfg(m=2, beta=3000, wide=5, min_sum=1000), p, 100, sl, 1))

    # windows clipped at bin 0 and at N - 1, in blocks that have neighbours on both sides with power where an unclipped
    # window would read on
    p = noise(rng, (1, 3, 64))
    for b in range(3):
        bump(p[0, b], 1, 2, 3000 + b)
        bump(p[0, b], 62, 2, 7000 + b)
    sl = {}
    for b in range(3):
        sl[(0, b, 0)] = (ACTIVE, 0, 3)
        sl[(0, b, 1)] = (ACTIVE, 1, 2)
        sl[(0, b, 2)] = (ACTIVE, 60, 63)
        sl[(0, b, 3)] = (TENTATIVE, 61, 62)
    out.append(Case("N64-edges", cfg(S=5, m=3, wide=7), p, 100, sl, 2))

    # a window across the guard (d = 3: bins 30 .. 34) with the capture's DC spike in it
    p = noise(rng, (1, 2, 64))
    for b in range(2):
        bump(p[0, b], 27, 2, 900)
        p[0, b, 31:34] += np.array([4000, 90000, 5000], np.uint64)
        bump(p[0, b], 37, 1, 700)
    out.append(Case("N64-guard", cfg(S=2, d=3, m=1, wide=9), p, 100, {(0, 0, 0): (ACTIVE, 25, 38), (0, 1, 1): (ACTIVE, 29, 35)}, 3))

    # first_bin == last_bin with m = 0: one bin is the peak, the centroid, both edges and all of the carrier
    p = noise(rng, (1, 1, 64))
    p[0, 0, 40] = 123456
    p[0, 0, 63] = 777
    p[0, 0, 0] = 555
    out.append(Case("N64-single-bin", cfg(S=4, m=0, wide=2), p, 100,
                    {(0, 0, 0): (ACTIVE, 40, 40), (0, 0, 1): (ACTIVE, 63, 63), (0, 0, 2): (ACTIVE, 0, 0), (0, 0, 3): (TENTATIVE, 41, 41)}, 4))

    # free, tentative, active and closing slots side by side; two slots whose windows overlap, two that are equal
    p = noise(rng, (1, 2, 64))
    for b in range(2):
        bump(p[0, b], 12, 4, 60000)
        bump(p[0, b], 20, 2, 30000)
        bump(p[0, b], 50, 3, 9000)
    sl = {(0, 0, 0): (ACTIVE, 8, 16), (0, 0, 1): (TENTATIVE, 14, 22), (0, 0, 2): (CLOSING, 47, 53), (0, 0, 3): (FREE, 0, 0),
          (0, 0, 5): (ACTIVE, 8, 16), (0, 0, 7): (CLOSING, 8, 16),
          (0, 1, 1): (ACTIVE, 47, 53), (0, 1, 4): (CLOSING, 10, 20), (0, 1, 6): (TENTATIVE, 11, 21)}
    out.append(Case("N64-states-overlap", cfg(S=8, m=2, wide=9), p, 100, sl, 5))

    # E = 0: nothing in the window is over the floor (bins at the floor among them); a window whose only excess is guarded
    p = noise(rng, (1, 1, 64), 80, 101)
    p[0, 0, 32] = 50000
    p[0, 0, 10] = 100
    out.append(Case("N64-empty", cfg(S=3, m=2, wide=5), p, 100, {(0, 0, 0): (ACTIVE, 8, 14), (0, 0, 1): (TENTATIVE, 31, 33), (0, 0, 2): (ACTIVE, 50, 50)}, 6))

    # every p = 2^32 - 1 with f = 0 and no guard: the largest sums, at both ends of N
    for N, name in ((64, "N64-saturated"), (2048, "N2048-saturated")):
        p = np.full((1, 1, N), M32, np.uint64)
        sl = {(0, 0, 0): (ACTIVE, 0, N - 1), (0, 0, 1): (ACTIVE, N // 2 - 9, N // 2 + 8)}
        out.append(Case(name, cfg(N=N, S=2, d=0, m=64, beta=32767, c=8, min_sum=M32, wide=N // 2 + 1), p, 0, sl, 7))

    # peak ties: the maximum twice and three times, the lowest bin counts; the carrier sits round that bin
    p = noise(rng, (1, 1, 64))
    p[0, 0, [20, 26]] = 9000
    p[0, 0, 21] = 3000
    p[0, 0, [44, 45, 50]] = 70000
    out.append(Case("N64-peak-ties", cfg(S=2, m=1, c=1, wide=30), p, 100, {(0, 0, 0): (ACTIVE, 18, 28), (0, 0, 1): (ACTIVE, 42, 52)}, 8))

    # beta = 0: the edges are the first and last bin with any excess (bins under the floor at both ends of the window);
    # beta = 32767: both edges close in on the middle
    p = noise(rng, (1, 1, 64), 80, 100)
    p[0, 0, 22:29] = [400, 900, 5000, 9000, 4000, 800, 300]
    p[0, 0, 40:44] = [1100, 1100, 1100, 1100]
    sl = {(0, 0, 0): (ACTIVE, 20, 30), (0, 0, 1): (ACTIVE, 40, 43)}
    out.append(Case("N64-beta0", cfg(S=2, m=2, beta=0, wide=8), p, 100, sl, 9))
    out.append(Case("N64-beta-max", cfg(S=2, m=2, beta=32767, wide=8), p, 100, sl, 10))

    # c = 0: the carrier is the peak bin alone; c = 8 with the peak one bin from the window's edge and power just outside
    # the window, inside the row
    p = noise(rng, (1, 1, 64))
    p[0, 0, 10:15] = [2000, 30000, 2500, 2600, 900]
    p[0, 0, 50:58] = [60000, 50000, 8000, 400, 300, 350, 500, 9000]
    p[0, 0, 46:50] = [20000, 20000, 20000, 20000]
    sl = {(0, 0, 0): (ACTIVE, 10, 14), (0, 0, 1): (ACTIVE, 50, 57)}
    out.append(Case("N64-carrier-c0", cfg(S=2, m=0, c=0, cq8=200, wide=30), p, 100, sl, 11))
    out.append(Case("N64-carrier-c8-edge", cfg(S=2, m=0, c=8, cq8=200, wide=30), p, 100, sl, 12))

    # min_sum just above and just below E: slot 0 has E = 5000 (not weak at min_sum 5000), slot 1 E = 4999 (weak)
    p = np.full((1, 1, 64), 100, np.uint64)
    p[0, 0, 10:13] = [1100, 3100, 1100]
    p[0, 0, 40:43] = [1100, 3099, 1100]
    out.append(Case("N64-minsum", cfg(S=2, m=1, min_sum=5000, wide=30), p, 100, {(0, 0, 0): (ACTIVE, 10, 12), (0, 0, 1): (ACTIVE, 40, 42)}, 13))

    # planted on both OBW edges: four bins of e = 100 and beta = 1/4, so 65536 L(lo) == beta E == 65536 R(hi): > moves both
    # edges in by one bin, >= would not
    p = np.full((1, 1, 64), 100, np.uint64)
    p[0, 0, 20:24] = 200
    out.append(Case("N64-obw-edge", cfg(S=1, m=0, beta=16384, wide=3), p, 100, {(0, 0, 0): (ACTIVE, 20, 23)}, 14))

    # the hint: a carrier (CARRIER), a flat narrow run (NARROW), a flat wide run (WIDE), a wide run with a carrier that has
    # half of the power (WIDE: the width is asked first), and the carrier again under min_sum (NONE)
    p = np.full((1, 2, 64), 100, np.uint64)
    p[0, :, 5:8] = [300, 9100, 300]
    p[0, 1, 6] = 8100
    p[0, :, 12:20] = 1300
    p[0, :, 22:34] = 1100
    p[0, :, 40:52] = 1100
    p[0, :, 45] = 30100
    sl = {(0, 0, 0): (ACTIVE, 5, 7), (0, 0, 1): (ACTIVE, 12, 19), (0, 0, 2): (ACTIVE, 22, 33), (0, 0, 3): (ACTIVE, 40, 51),
          (0, 1, 0): (ACTIVE, 5, 7), (0, 1, 3): (ACTIVE, 40, 51)}
    hints = Case("N64-hints", cfg(S=4, d=0, m=1, c=1, cq8=128, wide=10, min_sum=9000), p, 100, sl, 15)
    out.append(hints)

    out.append(random_case("N128-sources3", 128, 3, 3, 8, 16, m=5, beta=1000, c=2, min_sum=20000, wide=20))
    out.append(random_case("N256-random", 256, 1, 2, 5, 17, m=7, beta=328, c=1, min_sum=5000, wide=30))
    out.append(random_case("N512-random", 512, 2, 1, 4, 18, d=5, m=64, beta=5000, c=3, min_sum=5000, wide=64))
    out.append(random_case("N1024-random", 1024, 1, 2, 9, 19, d=2, m=11, beta=20000, c=8, min_sum=0, wide=65))
    out.append(random_case("N2048-S64", 2048, 1, 2, 64, 20, d=3, m=16, beta=328, c=4, min_sum=100000, wide=128))

    assert [x.name for x in out] == NAMES
    return out


# The three-station capture: an AM station (a carrier and its tone sidebands), a narrow FM station with voice-band deviation and a
# wide FM (broadcast) station from the project's synthetic sources, read at N = 2048, F = 4 (1 kHz bins).  What tests/test_measure_host.py
# holds the default thresholds to and what iqdemod_wide modes=auto is run on.
THREE = dict(N=2048, F=4, blocks=6, S=8)
THREE_STATIONS = [
    {"offset": -600e3, "kind": "am", "amplitude": 25.0, "tone": 3000.0, "depth": 0.5, "mode": "am"},
    {"offset": -100e3, "kind": "fm", "amplitude": 25.0, "tone": 1300.0, "deviation": 5000.0, "mode": "fm"},
    {"offset": 500e3, "kind": "wbfm", "amplitude": 25.0, "tone": 4000.0, "deviation": 75000.0, "mode": "wbfm"},
]
THREE_HINTS = {"am": mm.CARRIER, "fm": mm.NARROW, "wbfm": mm.WIDE}


def three_wide(blocks=None):
    """[1, bytes] uint8"""
    from rtlsdrdiags_amd import synth
    k = THREE
    n = k["N"] * k["F"] * (blocks or k["blocks"])
    return np.ascontiguousarray(synth.wideband(n, float(RATE), THREE_STATIONS, seed=41)).reshape(1, -1)


def auto_modes(slots, meas, per_call):
    """iqdemod_wide modes=auto on one source's tables [blocks, S], in calls of per_call blocks: the (first block of the call,
    slot, id, mode) the tool sets, in its order - per slot the id of the call's last active block, if not decided yet; the
    hint most of the call's blocks with that id active give, ties to the lowest; no hint: fm"""
    out, decided = [], {}
    for b0 in range(0, len(slots), per_call):
        sl, ms = slots[b0:b0 + per_call], meas[b0:b0 + per_call]
        for c in range(slots.shape[1]):
            ids = [int(x["track_id"]) for x in sl[:, c] if x["state"] == 2]
            if not ids or decided.get(c) == ids[-1]:
                continue
            votes = [0, 0, 0, 0]
            for x, y in zip(sl[:, c], ms[:, c]):
                if x["state"] == 2 and x["track_id"] == ids[-1]:
                    votes[int(y["hint"])] += 1
            hint = 0
            for h in (1, 2, 3):
                if votes[h] > (votes[hint] if hint else 0):
                    hint = h
            decided[c] = ids[-1]
            out.append((b0, c, ids[-1], {0: 2, 1: 1, 2: 2, 3: 3}[hint]))
    return out
