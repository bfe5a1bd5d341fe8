"""The inputs of tests/test_gpu_filter.py, proven against the defects of filter_model.py by tests/test_filter_host.py.
Every case is small (at most 8192 samples per channel).  Named after the shape at which the kernels can go wrong:

  channels   1, 63, 64, 65 (a partial last wave of the IIR, a last workgroup of the FIR with idle groups), 300
  taps       1 (no history at all), 2, 8, 31, 40, 300 (calls shorter than the history), 1024 (the largest lead-in)
  factor     1, 2, 3, 4, 5, 64; calls of factor - 1 samples that yield no output
  IIR order  (1,1) (2,1) (3,2): registers; (4,3) (64,64): the rings in LDS
  calls      [0, 1, 2, 5, 700, 701, 1999, N]; T - 1, T, T + 1 samples for T = iqd_filter_tile_samples (256 factor for the
             FIR kinds: 255 outputs run as four groups of 64 lanes, 256 as one group, 257 as two; 64 steps for the IIR);
             chains of 1-sample calls longer than the history; rows of 16 k bytes from an aligned base (the 16-byte
             staging) and rows that are not
  Q15        rails with taps of amplitude 0.9 (the clamp fires mid-sum), tap sets with K0 = L (never a clamp), a set with
             0 < K0 < L and K0 odd (both parts of the sum in one output, the odd tap on the clamped side)"""
import os
from collections import namedtuple

import numpy as np

import filter_model as fm

Case = namedtuple("Case", "name kind num den factor x cuts blind")
STD_CUTS = [0, 1, 2, 5, 700, 701, 1999]
T_FIR, T_IIR = 256, 64              # iqd_filter_tile_samples: T_FIR x factor, T_IIR (test_filter_host.py checks both)


def rails(rng, shape):
    return np.where(rng.random(shape) < 0.5, -32768, 32767).astype(np.int16)


def stable_iir(rng, n_num, n_den, radius=0.98):
    """random numerator; denominator from conjugate pole pairs (and one real pole if n_den is odd) of modulus <= radius,
    multiplied out in float64 and rounded to float32; returned without its leading 1"""
    poly = np.array([1.0])
    for _ in range(n_den // 2):
        r, th = radius * rng.random() ** 0.5, np.pi * rng.random()
        poly = np.convolve(poly, [1.0, -2 * r * np.cos(th), r * r])
    if n_den % 2:
        poly = np.convolve(poly, [1.0, -radius * (2 * rng.random() - 1)])
    return rng.normal(0, 0.5, n_num).astype(np.float32), poly[1:].astype(np.float32)


def cuts_to(n, cuts):
    return [c for c in cuts if c < n] + [n]


def build(oracle, golden):
    rng = np.random.default_rng(20)
    g = golden["primitives"]
    cases = []

    def add(name, kind, num, den, factor, x, cuts, blind=()):
        x = np.atleast_2d(x)
        assert x.shape[1] <= 8192
        cases.append(Case(name, kind, np.asarray(num, np.float32), None if den is None else np.asarray(den, np.float32),
                          factor, x, cuts_to(x.shape[1], cuts), dict(blind)))

    i16 = lambda n_ch, n: rng.integers(-32768, 32768, (n_ch, n)).astype(np.int16)
    f32 = lambda n_ch, n: rng.normal(0, 5000, (n_ch, n)).astype(np.float32)
    one_by_one = lambda n: list(range(n))
    FREE = {"clamp_end": "sum |hq| <= 32767: no clamp can fire", "clamp_hi": "sum |hq| <= 32767: no clamp can fire"}

    # ---- Q15, clamp-reaching ----
    add("dec-rails-L24-f3", "decimate_i16", rng.uniform(-0.9, 0.9, 24), None, 3, rails(rng, 600), [0, 0, 2, 4, 5, 300],      # (an empty call, then calls of factor - 1 samples)
        blind={"chan0": "one channel"})
    add("dec-audio40-xsat", "decimate_i16", oracle.taps_f32("audio40"), None, 2, g["xsat"], STD_CUTS,
        blind={"chan0": "one channel", "taps_rev": "the taps are symmetric"})
    add("fir-hilbert-xsat", "fir_i16", oracle.taps_f32("ssb_hilbert"), None, 1, g["xsat"], STD_CUTS,
        blind={"chan0": "one channel"})
    h = np.full(40, 0.21, np.float32) * np.where(np.arange(40) % 3 == 0, -1, 1)     # |hq| = 6881 each, but
    h[0] = 0.1                                                                   # 3277 + 4 x 6881 = 30801 <= 32767 < + 6881: K0 = 5
    add("dec-k0-inside-L40-f5", "decimate_i16", h, None, 5, rails(rng, (2, 1283)), [0, 4, 8, 9, 1280])
    add("dec-rails-L1024-f3", "decimate_i16", rng.uniform(-0.9, 0.9, 1024), None, 3, rails(rng, 4000), [0, 5, 1024],
        blind={"chan0": "one channel", "no_round": "1024 taps of amplitude 0.9 on the rails: every sum meets the clamp on its way, which forgets the offset"})
    add("fir-rails-L300-65ch", "fir_i16", rng.uniform(-0.9, 0.9, 300), None, 1, rails(rng, (65, 1999)), STD_CUTS)
    # ---- Q15, clamp-free (K0 = L) ----
    add("dec-wbfm_d1-63ch-tiles", "decimate_i16", oracle.taps_f32("wbfm_d1"), None, 4, i16(63, 3100),
        [0, 4 * T_FIR - 1, 8 * T_FIR - 1, 12 * T_FIR], blind=dict(FREE, taps_rev="the taps are symmetric"))
    add("dec-am_s1-64ch-aligned", "decimate_i16", oracle.taps_f32("am_s1"), None, 4, i16(64, 1000), [0, 8, 16, 24, 504],
        blind=dict(FREE, taps_rev="the taps are symmetric"))
    hr = rng.uniform(-1, 1, 31)
    add("fir-free-L31-65ch", "fir_i16", hr * 0.99 / np.abs(hr).sum(), None, 1, i16(65, 701), [0, 1, 2, 5, 700], blind=FREE)
    add("dec-L1-f64-300ch", "decimate_i16", [0.5], None, 64, i16(300, 64 * 5 + 7), [0, 63, 126, 189, 190],
        blind={"taps_rev": "one tap", "hist_zero": "one tap: no history", "chan0": "one tap: no history",
               "clamp_end": "one tap", "clamp_hi": "|acc| <= 2^29"})
    add("dec-L2-f2-1sample", "decimate_i16", [0.75, -0.5], None, 2, rails(rng, (3, 40)), one_by_one(40),
        blind={"clamp_end": "two taps, and 2^14 + 0.75 x 2^30 is inside the range: only the last clamp can fire"})
    add("fir-L8-1sample", "fir_i16", rng.uniform(-0.9, 0.9, 8), None, 1, i16(2, 30), one_by_one(30))
    # ---- float FIR ----
    add("f32-L48-300ch", "fir_f32", rng.normal(0, 0.2, 48), None, 1, f32(300, 2048), [0, 1001])
    add("f32-L1024-tiles", "fir_f32", rng.normal(0, 0.05, 1024), None, 1, f32(1, 1500), [0, T_FIR - 1, 2 * T_FIR - 1, 3 * T_FIR],
        blind={"chan0": "one channel"})
    add("f32-L1-63ch", "fir_f32", [0.3], None, 1, f32(63, 130), [0, 1, 65],
        blind={"taps_rev": "one tap", "desc_k": "one tap", "hist_zero": "one tap: no history", "chan0": "one tap: no history",
               "fma": "0 + h x rounds once either way"})
    add("f32-L2-64ch-1sample", "fir_f32", [0.3, -1.7], None, 1, f32(64, 12), one_by_one(12),
        blind={"desc_k": "two terms: the first sum is exact from 0, the addition commutes"})
    add("f32-L31-65ch", "fir_f32", rng.normal(0, 0.3, 31), None, 1, f32(65, 1999), STD_CUTS)
    # ---- IIR ----
    add("iir-1-1", "iir_f32", [0.7], [-0.9], 1, f32(1, 2000), STD_CUTS,
        blind={"taps_rev": "one coefficient each", "desc_k": "one term each", "fma": "one term each: 0 + p rounds once either way",
               "chan0": "one channel"})
    add("iir-dcblock-300ch-tiles", "iir_f32", [1.0, -1.0], [-0.95], 1, f32(300, 700), [0, T_IIR - 1, 2 * T_IIR - 1, 3 * T_IIR],
        blind={"desc_k": "two terms: the first sum is exact from 0, the addition commutes",
               "fma": "the products by 1 and -1 are exact and the recursive sum has one term"})
    b, a = stable_iir(rng, 3, 2)
    add("iir-biquad-65ch-1sample", "iir_f32", b, a, 1, f32(65, 701), one_by_one(10) + [700])
    b, a = stable_iir(rng, 4, 3)
    add("iir-4-3-64ch", "iir_f32", b, a, 1, f32(64, 500), [0, 1, 2, 5, 64, 65])
    b, a = stable_iir(rng, 64, 64, radius=0.5)
    add("iir-64-64-63ch", "iir_f32", b, a, 1, f32(63, 300), [0, 1, 2, 5, 63, 200])
    imp = np.zeros((2, 200), np.float32)
    imp[0, 0], imp[1, 0] = 1.0, -1.0
    add("iir-subnormal-decay", "iir_f32", [1.0], [0.5], 1, imp, [0, 1, 100, 140],
        blind={"taps_rev": "one coefficient each", "desc_k": "one term each", "fma": "one term each: 0 + p rounds once either way"})
    return cases


def oracle_run(oracle, c, ch):
    """channel ch of a case through oracle/libiqd_oracle.so, from the zero state in one piece - or None where the oracle's
    fixed-size filters cannot hold the case (Q15: 40 taps; IIR: 8 and 4 coefficients).  iqo_fir_q15 has no Python wrapper:
    it is called through oracle.lib."""
    import ctypes as C
    x = np.ascontiguousarray(c.x[ch])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    if c.kind in fm.Q15_KINDS:
        if len(c.num) > 40:
            return None
        if c.kind == "decimate_i16":
            return oracle.decimate_q15(c.num, c.factor, x)
        out = np.zeros(len(x), np.int16)
        oracle.lib.iqo_fir_q15(ptr(c.num), len(c.num), ptr(x), len(x), ptr(out))
        return out
    if c.kind == "fir_f32":          # iqo_fir_f32 holds 8 taps; the float decimator at factor 1 is the same sum for any length
        return oracle.fir_f32(c.num, x) if len(c.num) <= 8 else oracle.decimate_f32(c.num, 1, x)
    if len(c.num) > 8 or len(c.den) > 4:
        return None
    return oracle.iir_f32(c.num, c.den, x)


def reference_run(reference, c, ch):
    """channel ch of a case through the unmodified reference classes (oracle/_ref), any size"""
    x = c.x[ch]
    if c.kind == "decimate_i16":
        return reference.decimate_q15(c.num, c.factor, x)
    if c.kind == "fir_i16":
        return reference.fir_q15(c.num, x)
    if c.kind == "fir_f32":
        return reference.fir_f32(c.num, x)
    return reference.iir_f32(c.num, c.den, x)


def load():
    """the cases, built from the repository's own oracle library and golden vectors"""
    from oracle import bindings
    root = os.path.dirname(os.path.abspath(__file__))
    golden = {"primitives": np.load(os.path.join(root, "golden", "primitives.npz"))}
    return build(bindings.Oracle(), golden)
