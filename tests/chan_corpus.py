"""A directed corpus of small channelizer cases: inputs found by searching the spec's own intermediate values, so that
every step of include/iqdemod.h's integer spec shows in the output bytes (tests/chan_mutants.py holds the defects each
family must expose; tests/test_chan_corpus_host.py checks that it does, tests/test_gpu_chan_corpus.py runs it).

cases(P, default_taps) -> [Case]: one channel each (M, h, inc, L), its wideband bytes from sample 0, and call cuts in units of 64 M
bytes (the shortest call).  Everything is deterministic: fixed seeds, and searches that take the first hit in a fixed
order.  Families:
  final_tie   K = 1 (the tap is unrotated, so the two bytes of sample n set ar, ai freely): per output the byte pair that
              puts rr or ri exactly on the final rounding's tie, unsaturated, at every L, on both rails and both signs
  a_tie_1tap  K = 1, g = 128: A = 128 x, a tie of stage a for every odd x
  low_order   small taps, low-amplitude input, L >= 6, K at the edges of the padding to 32 and of the two A-operand
              paths (K <= 256: registers, K > 256: read per group), M even and odd: input samples steered so that
              A = 128 and 127 (mod 256) occur on both rails; history carried over many shortest calls
  sat16       sum |h| at the bound 256 sum |h| = 2^31 - 256, sign-matched full-scale input at 0 degrees and on the
              45-degree diagonals: both int16 rails, the value just past a rail, and the largest |A| the bound allows
  tap_edges   h = +-32639 on phasor entries +-32767 and 0, g whose lo byte is -128 and +127, g past +-32512
  general     default taps with full-scale stretches (both byte rails), and calls of several windows with a 32-output
              tail"""
import numpy as np

from tests import chan_model as cm

BOUND_SUM = (2 ** 31 - 256) // 256          # sum |h| at the bound: 8388607
K_EDGES = (31, 32, 33, 255, 256, 257, 1023, 1024)


class Case:
    def __init__(self, name, family, M, h, inc, L, wide, cuts, note=""):
        self.name, self.family, self.M, self.inc, self.L, self.note = name, family, int(M), int(inc), int(L), note
        self.h = np.asarray(h, np.int16)
        self.wide = np.ascontiguousarray(wide, np.uint8)
        unit = 64 * self.M
        assert len(self.wide) % unit == 0 and sum(cuts) == len(self.wide) // unit, (name, len(self.wide), sum(cuts))
        self.cuts = [int(c) for c in cuts]
        assert np.abs(self.h.astype(np.int64)).max() <= 32639 and np.abs(self.h.astype(np.int64)).sum() <= BOUND_SUM

    @property
    def K(self):
        return len(self.h)

    @property
    def n_out(self):
        return len(self.wide) // (2 * self.M)

    @property
    def path(self):
        """the kernel's code path: A operands in registers or read per group, windows 4- or 2-byte aligned"""
        return ("K<=256" if self.K <= 256 else "K>256") + (", M even" if self.M % 2 == 0 else ", M odd")

    def __repr__(self):
        return "%s (M=%d K=%d inc=0x%08x L=%d, %d outputs, cuts %s)" % (self.name, self.M, self.K, self.inc, self.L,
                                                                       self.n_out, self.cuts)


def _cuts(units, ones, seed):
    """`ones` shortest calls first (history carried across them), then uneven calls to the end"""
    rng = np.random.default_rng(seed)
    out = [1] * min(ones, units)
    while sum(out) < units:
        out.append(int(min(units - sum(out), rng.integers(1, 6))))
    return out


def _phasor_at(P, n, inc):
    i = ((int(n) * int(inc)) % (1 << 32)) >> 20
    return int(P[i][0]), int(P[i][1])


# ---------------------------------------------------------------------------------------------------- final ties
# (h, M, inc) per L: the first of these whose 256 x 256 search per output covers both rails and both signs
_TIE_TRIES = [(20000, 4, 0x01234567), (256, 4, 0x01234567), (32639, 4, 0x01234567), (12345, 3, 0x3039a1b7),
              (29000, 4, 0x0badcafe), (31000, 5, 0x2468ace1), (27183, 2, 0x01234567), (32001, 7, 0x13572468)]


_TIE_OUTPUTS = {0: 768, 1: 512, 2: 256}      # a tie is one pair in 2^(22-L) / 65536 per rail: more outputs at small L


def final_tie_search(P, hv, M, inc, L, n_out, seed):
    """wide bytes of a K = 1 case whose output m sits on the final rounding's tie wherever a byte pair allows it, and
    the number of unsaturated ties per class {(rail, sign)}"""
    rng = np.random.default_rng(seed)
    wide = rng.integers(0, 256, 2 * M * n_out, dtype=np.uint8)
    gr = (hv * int(P[0][0]) + (1 << 14)) >> 15            # k = 0: P[0] = (32767, 0), gi = 0
    x = np.arange(-128, 128, dtype=np.int64)
    a = np.clip((gr * x + 128) >> 8, -32768, 32767)
    sh, rnd = 22 - L, 1 << (21 - L)
    found = {(r, s): 0 for r in (0, 1) for s in (-1, 1)}
    for m in range(n_out):
        n = m * M + M - 1
        c, s = _phasor_at(P, n, inc)
        rr = a[:, None] * c + a[None, :] * s              # [xr index][xi index]
        ri = a[None, :] * c - a[:, None] * s
        ties = {}                                         # class -> the first unsaturated tie, in index order
        for rail, r in ((0, rr), (1, ri)):
            for i, j in np.argwhere(((r + rnd) & ((1 << sh) - 1)) == 0):
                v = int(r[i, j])
                if v != 0 and -127 <= (v + rnd) >> sh <= 127:
                    ties.setdefault((rail, 1 if v > 0 else -1), (int(i), int(j)))
        hit = None
        for j in range(4):                                # the class wanted first rotates with m
            cls = (m + j) % 4
            key = (cls & 1, 1 if cls & 2 else -1)
            if key in ties:
                hit = key + ties[key]
                break
        if hit:
            found[(hit[0], hit[1])] += 1
            wide[2 * n], wide[2 * n + 1] = hit[2], hit[3]   # byte = x + 128 = the index
    return wide, found


def _final_ties(P):
    out = []
    for L in range(9):
        best = None
        for t, (hv, M, inc) in enumerate(_TIE_TRIES):
            wide, found = final_tie_search(P, hv, M, inc, L, _TIE_OUTPUTS.get(L, 128), seed=100 + L)
            score = sum(1 for v in found.values() if v)
            if best is None or score > best[0]:
                best = (score, hv, M, inc, wide, found)
            if score == 4:
                break
        score, hv, M, inc, wide, found = best
        c = Case("final_tie_L%d" % L, "final_tie", M, [hv], inc, L, wide, _cuts(len(wide) // (64 * M), 2, L),
                 note="unsaturated ties per (rail, sign): %s" % sorted(found.items()))
        c.ties = found
        out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------- stage a
def _a_tie_one_tap():
    out = []
    for M, inc, L in ((4, 0x01234567, 8), (3, 0xfedcba98, 7)):
        rng = np.random.default_rng(200 + M)
        wide = (128 + rng.integers(-40, 41, 2 * M * 128)).astype(np.uint8)
        out.append(Case("a_tie_1tap_M%d" % M, "a_tie_1tap", M, [128], inc, L, wide, _cuts(len(wide) // (64 * M), 3, M)))
    return out


def steer(P, h, M, inc, wide, amp, residues=(128, 127)):
    """Walks the outputs in order and moves one rail of one of the newest M samples (they reach no earlier output) so
    that A = residue (mod 256) on the rail whose turn it is; returns the steered bytes."""
    gr, gi = cm.channel_taps(h, inc, P)
    K = len(h)
    x = np.asarray(wide, np.int64).reshape(-1, 2) - 128
    n_out = len(x) // M
    vals = np.arange(-amp, amp + 1, dtype=np.int64)
    for m in range(n_out):
        n = m * M + M - 1
        kk = min(K, n + 1)
        wr, wi = x[n - kk + 1:n + 1, 0][::-1], x[n - kk + 1:n + 1, 1][::-1]      # x[n - k], k = 0 ..
        rail, want = m & 1, residues[(m >> 1) % len(residues)]
        A = int(gr[:kk] @ wr - gi[:kk] @ wi) if rail == 0 else int(gr[:kk] @ wi + gi[:kk] @ wr)
        done = False
        for k0 in range(min(M, kk)):
            # d A / d x: rail 0: (gr, -gi) by (xr, xi); rail 1: (gi, gr)
            for comp, coef in ((0, gr[k0] if rail == 0 else gi[k0]), (1, -gi[k0] if rail == 0 else gr[k0])):
                if coef == 0:
                    continue
                new = A + int(coef) * (vals - x[n - k0, comp])
                ok = np.flatnonzero(new % 256 == want)
                if len(ok):
                    x[n - k0, comp] = vals[ok[0]]
                    done = True
                    break
            if done:
                break
    return (x + 128).astype(np.uint8).reshape(-1)


def _low_order(P):
    out = []
    plan = [(31, 63, 8), (32, 64, 8), (33, 5, 6), (255, 8, 8), (256, 63, 7), (257, 64, 8), (257, 3, 8), (1023, 63, 8),
            (1023, 4, 7), (1024, 2, 8), (1024, 64, 6), (1024, 5, 8), (33, 2, 8), (256, 7, 8)]
    for i, (K, M, L) in enumerate(plan):
        rng = np.random.default_rng(300 + i)
        hmax = 300 if K <= 33 else 100 if K <= 257 else 30
        h = rng.integers(-hmax, hmax + 1, K).astype(np.int16)
        h[0], h[-1] = 1 + i % 3, -(2 + i % 5)                   # odd and small newest tap: every residue reachable
        inc = int(rng.integers(1, 2 ** 32))
        kp = (K + 31) // 32 * 32
        carry = -(-kp // (32 * M))                              # shortest calls it takes to fill the history
        units = max(4, carry + 4) if M < 32 else 3
        amp = 6
        wide = (128 + rng.integers(-amp, amp + 1, 64 * M * units)).astype(np.uint8)
        wide = steer(P, h, M, inc, wide, amp)
        out.append(Case("low_order_K%d_M%d" % (K, M), "low_order", M, h, inc, L, wide, _cuts(units, carry + 2, i)))
    return out


def bound_taps(kind):
    """sum |h| exactly at the bound.  "0deg": 1024 taps; "45deg": the odd taps of 1024 (increment 2^29: tap k at k x 45
    degrees, the odd ones on the diagonals where |gr| + |gi| is largest)."""
    h = np.zeros(1024, np.int64)
    if kind == "0deg":
        h[:] = 8192
        h[-1] = 8191
    else:
        h[1::2] = 16384
        h[-1] = 16383
    assert np.abs(h).sum() == BOUND_SUM
    return h.astype(np.int16)


def over_bound_taps(kind):
    h = bound_taps(kind).copy()
    h[-1] += 1
    return h


def _sat16(P):
    out = []
    M, K, seg = 8, 1024, 160                                     # outputs per segment: the window fills after 128
    for kind, inc in (("0deg", 0), ("45deg", 1 << 29)):
        h = bound_taps(kind)
        gr, gi = cm.channel_taps(h, inc, P)
        rows = []
        # the sample at distance k behind an output is j = n - k, n = 7 (mod 8): k = (7 - j) mod 8 in the taps' period 8
        j = np.arange(M * seg)
        k = (7 - j) % 8
        # period-8 signs of the taps (all of one residue share a sign: h >= 0 and the phase repeats every 8 taps)
        sr = np.array([np.sign(gr[r::8].sum()) for r in range(8)])[k]
        si = np.array([np.sign(gi[r::8].sum()) for r in range(8)])[k]

        def full(sign):      # the byte that takes x to the rail of that sign (0: centre)
            return np.where(sign > 0, 255, np.where(sign < 0, 0, 128)).astype(np.uint8)

        for target in ("Ar-", "Ar+", "Ai-", "Ai+", "Ar just past +", "Ar at -"):
            if target.startswith("Ar j") or target.startswith("Ar a"):
                one = 1 if "+" in target else -1                # |x| = 1: A = +-sum |g| sits next to the int16 rail
                xr, xi = one * sr, -one * si
                seg_bytes = np.stack([128 + xr, 128 + xi], 1).astype(np.uint8)
            else:
                d = -1 if target[2] == "-" else 1
                if target[1] == "r":                            # Ar = sum gr xr - gi xi
                    seg_bytes = np.stack([full(d * sr), full(-d * si)], 1)
                else:                                           # Ai = sum gr xi + gi xr
                    seg_bytes = np.stack([full(d * si), full(d * sr)], 1)
            rows.append(seg_bytes.reshape(-1))
        wide = np.concatenate(rows)
        units = len(wide) // (64 * M)
        for L in (0, 5):
            out.append(Case("sat16_%s_L%d" % (kind, L), "sat16", M, h, inc, L, wide, _cuts(units, 6, L),
                            note="segments " + "Ar-, Ar+, Ai-, Ai+, Ar just past +, Ar at -"))
    return out


def _tap_edges(P):
    out = []
    # d = 2^30: tap k on phasor entry k x 1024: (32767, 0), (0, 32767), (-32767, 0), (0, -32767)
    h = [32639, 32639, -32639, -32639, 128, -128, 127, -129, 32384, -32384, 32639, -32639, 32513, -32513, 255, -257]
    for i, (M, inc, L, amp) in enumerate(((4, 1 << 30, 3, 4), (5, 1 << 30, 2, 127), (2, 0, 4, 5),
                                          (3, 0x01234567, 3, 6))):
        rng = np.random.default_rng(500 + i)
        wide = (128 + rng.integers(-amp, amp + 1, 2 * M * 256)).astype(np.uint8)
        out.append(Case("tap_edges_%d" % i, "tap_edges", M, h, inc, L, wide, _cuts(len(wide) // (64 * M), 2, i)))
    # the same extremes inside a filter of the per-group path
    rng = np.random.default_rng(510)
    hl = rng.integers(-40, 41, 300).astype(np.int16)
    hl[[0, 7, 64, 128, 255, 256, 299]] = [32639, -32639, 32639, -32639, 128, -129, 32639]
    wide = (128 + rng.integers(-3, 4, 2 * 7 * 128)).astype(np.uint8)
    out.append(Case("tap_edges_K300", "tap_edges", 7, hl, 0x40000000, 4, wide, _cuts(len(wide) // (64 * 7), 3, 9)))
    return out


def _general(P, default_taps):
    out = []

    def stream(rng, n_bytes):
        u = rng.integers(0, 256, n_bytes, dtype=np.uint8)
        q = n_bytes // 4 // 2 * 2
        u[q:2 * q], u[2 * q:3 * q] = 0xFF, 0x00
        return u

    # several windows per call with a 32-output tail: t_max = 1024 (M = 8, K = 105), 192 (M = 64, K = 1024)
    rng = np.random.default_rng(600)
    M = 8
    n_out = 2 * 1024 + 32
    out.append(Case("general_windows_tail32_M8", "general", M, default_taps(M), 0x9e3779b9, 8, stream(rng, 2 * M * n_out),
                    [n_out // 32], note="one call: windows of 1024, 1024 and 32 outputs"))
    M = 64
    n_out = 2 * 192 + 32
    h = rng.integers(-6000, 6001, 1024).astype(np.int16)
    out.append(Case("general_windows_tail32_M64", "general", M, h, 0x7f4a7c15, 1, stream(rng, 2 * M * n_out),
                    [7, 6], note="calls of 224 and 192 outputs: windows of 192 + 32, and exactly one window"))
    M = 33
    out.append(Case("general_default_M33", "general", M, default_taps(M), 0xdeadbeef, 8, stream(rng, 64 * M * 10),
                    _cuts(10, 3, 33)))
    return out


def cases(P, default_taps):
    """default_taps(M) -> the library's default prototype (capi.channelizer_default_taps: host only)."""
    return _final_ties(P) + _a_tie_one_tap() + _low_order(P) + _sat16(P) + _tap_edges(P) + _general(P, default_taps)
