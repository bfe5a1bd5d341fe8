"""CPU tier of the stand-alone filters (include/iqdemod.h: iqd_filter_*): the numpy model of tests/filter_model.py against
the oracle and the unmodified reference on every GPU input of tests/filter_cases.py, the mutation proof of those inputs,
the two host-only functions, and the code object of iqd_filter.hip.

Where the three yardsticks reach:
  * oracle/libiqd_oracle.so holds Q15 filters of up to 40 taps and IIRs of up to 8 and 4 coefficients; longer cases are
    pinned by the reference alone (and by the model's agreement with both below those sizes).
  * The reference's IirFilter agrees with the specified recurrence r = sum den[k] y[n-1-k] for n_den = 1 - every use the
    reference makes of it.  For n_den >= 2 its ring starts the sum at the OLDEST output (IirFilter.cc:199-229 reads from
    ringBufferIndex, which shiftSampleIn :250-266 has already advanced): den[0] meets y[n-n_den].  The interface follows the
    specified recurrence, which is the oracle's; test_reference_iir_ring_order pins what the reference does instead."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import filter_cases as fc
import filter_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_CODE = {"decimate_i16": 0, "fir_i16": 1, "fir_f32": 2, "iir_f32": 3}


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def cases(oracle, golden):
    return fc.build(oracle, golden)


@pytest.fixture(scope="module")
def wants(cases):
    """the model's output of every case, in the case's calls: computed once"""
    return {c.name: fm.run(c.kind, c.num, c.den, c.factor, c.x, c.cuts) for c in cases}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def some_channels(c):
    n = c.x.shape[0]
    return sorted({0, n // 2, n - 1} | set(range(0, n, 37)))


def test_model_quantises_like_the_oracle(oracle):
    import ctypes as C
    rng = np.random.default_rng(1)
    h = np.concatenate([rng.uniform(-1, 1, 500), [1.0, -1.0, 0.5 / 32768, -0.5 / 32768, 1.5 / 32768, 0.99998]]).astype(np.float32)
    hq = np.zeros(len(h), np.int16)
    oracle.lib.iqo_quantize_taps(h.ctypes.data_as(C.c_void_p), len(h), hq.ctypes.data_as(C.c_void_p))
    assert np.array_equal(fm.quantize(h), hq)
    assert fm.quantize([1.0])[0] == -32768


def test_model_equals_the_oracle_on_every_case(oracle, cases, wants):
    checked = 0
    for c in cases:
        assert np.array_equal(bits(wants[c.name]), bits(fm.run(c.kind, c.num, c.den, c.factor, c.x))), c.name   # cuts change nothing
        for ch in some_channels(c):
            got = fc.oracle_run(oracle, c, ch)
            if got is None:
                assert (c.kind in fm.Q15_KINDS and len(c.num) > 40) or (c.kind == "iir_f32" and (len(c.num) > 8 or len(c.den) > 4))
                continue
            assert got.dtype == wants[c.name].dtype and np.array_equal(bits(got), bits(wants[c.name][ch])), (c.name, ch)
            checked += 1
    assert checked >= len(cases)


def test_model_equals_the_reference_on_every_case(reference, cases, wants):
    for c in cases:
        if c.kind == "iir_f32" and len(c.den) > 1:
            continue                                       # the reference's ring order: see the module's docstring
        for ch in some_channels(c)[:3]:
            got = fc.reference_run(reference, c, ch)
            assert np.array_equal(bits(got), bits(wants[c.name][ch])), (c.name, ch)


def test_reference_iir_ring_order(reference):
    """n_den = 2: the reference multiplies den[0] with y[n-2] and den[1] with y[n-1], in that order"""
    rng = np.random.default_rng(5)
    b, a = np.float32([0.5, 0.25]), np.float32([-0.6, 0.3])
    x = rng.normal(0, 100, 64).astype(np.float32)
    y, x1, y1, y2 = np.zeros(64, np.float32), np.float32(0), np.float32(0), np.float32(0)
    for n in range(64):
        v = np.float32(0) + b[0] * x[n]
        v = v + b[1] * x1
        r = np.float32(0) + a[0] * y2
        r = r + a[1] * y1
        y[n] = v - r
        x1, y2, y1 = x[n], y1, y[n]
    assert np.array_equal(bits(reference.iir_f32(b, a, x)), bits(y))
    assert not np.array_equal(bits(y), bits(fm.run("iir_f32", b, a, 1, x)[0]))


def test_every_gpu_input_sees_every_defect(cases, wants):
    seen = {k: set() for k in KIND_CODE}
    for c in cases:
        assert all(d in fm.DEFECTS and fm.applies(d, c.kind) and why for d, why in c.blind.items()), c.name
        for d in fm.DEFECTS:
            if not fm.applies(d, c.kind):
                continue
            same = np.array_equal(bits(wants[c.name]), bits(fm.run(c.kind, c.num, c.den, c.factor, c.x, c.cuts, defect=d)))
            assert same == (d in c.blind), (c.name, d, "not exposed" if same else "listed as blind but exposed")
            if not same:
                seen[c.kind].add(d)
    for kind in KIND_CODE:
        assert seen[kind] == {d for d in fm.DEFECTS if fm.applies(d, kind)}, (kind, seen[kind])
    assert set().union(*seen.values()) == set(fm.DEFECTS)


def test_the_cases_reach_what_they_are_for(oracle, cases, wants):
    by = {c.name: c for c in cases}
    assert {c.x.shape[0] for c in cases} >= {1, 63, 64, 65, 300}
    assert {len(c.num) for c in cases if c.kind != "iir_f32"} >= {1, 2, 8, 31, 40, 300, 1024}
    assert {c.factor for c in cases} >= {1, 2, 3, 4, 5, 64}
    assert {(len(c.num), len(c.den)) for c in cases if c.kind == "iir_f32"} >= {(1, 1), (2, 1), (3, 2), (4, 3), (64, 64)}
    assert all(c.x.shape[1] <= 8192 for c in cases)
    assert any(c.cuts[:7] == fc.STD_CUTS for c in cases if c.kind in fm.Q15_KINDS)
    assert any(c.cuts[:7] == fc.STD_CUTS for c in cases if c.kind == "fir_f32")
    assert any(c.cuts[:7] == fc.STD_CUTS for c in cases if c.kind == "iir_f32")
    lens = lambda c: [b - a for a, b in zip(c.cuts[:-1], c.cuts[1:])]
    for kind in KIND_CODE:                                  # T - 1, T, T + 1
        hit = False
        for c in cases:
            if c.kind == kind or (kind == "fir_i16" and c.kind == "decimate_i16"):
                t = (fc.T_IIR if kind == "iir_f32" else fc.T_FIR * c.factor)
                hit = hit or lens(c)[:3] == [t - 1, t, t + 1]
        assert hit, kind
    for c in cases:                                         # a chain of 1-sample calls longer than the history
        if lens(c)[:8] == [1] * 8:
            state = len(c.num) - 1 + (len(c.den) if c.den is not None else 0)
            assert sum(1 for n in lens(c) if n == 1) > state, c.name
    assert {c.kind for c in cases if lens(c)[:8] == [1] * 8} == set(KIND_CODE)
    c = by["dec-L1-f64-300ch"]                              # calls of factor - 1 samples: the first yields nothing
    assert lens(c)[:3] == [63, 63, 63] and c.cuts[1] // 64 == 0
    assert any(c.x.shape[1] * c.x.itemsize % 16 == 0 for c in cases) and any(c.x.shape[1] * c.x.itemsize % 16 for c in cases)
    c = by["dec-am_s1-64ch-aligned"]                        # every call a whole number of 16-byte units
    assert all(n * 2 % 16 == 0 for n in c.cuts)
    # Q15: the clamp fires mid-sum in the rails cases, never in the clamp-free ones; K0 inside (0, L) and odd in one case
    k0 = {c.name: fm.clamp_free_taps(fm.quantize(c.num)) for c in cases if c.kind in fm.Q15_KINDS}
    for name in ("dec-wbfm_d1-63ch-tiles", "dec-am_s1-64ch-aligned", "fir-free-L31-65ch"):
        assert k0[name] == len(by[name].num), name
    assert k0["dec-k0-inside-L40-f5"] == 5 and len(by["dec-k0-inside-L40-f5"].num) == 40
    c = by["dec-rails-L24-f3"]
    late = fm.run(c.kind, c.num, None, c.factor, c.x, c.cuts, defect="clamp_end")
    assert np.count_nonzero(late != wants[c.name]) > wants[c.name].size // 4
    for name in ("dec-audio40-xsat", "fir-hilbert-xsat", "dec-k0-inside-L40-f5"):
        c = by[name]
        assert "clamp_end" not in c.blind and 0 < k0[name] < len(c.num)
    # IIR: finite in, finite out; the decay passes through the subnormals and ends at a signed zero
    for c in cases:
        if c.kind == "iir_f32":
            assert np.isfinite(c.x).all() and np.isfinite(wants[c.name]).all(), c.name
    c = by["iir-subnormal-decay"]
    y = fc.oracle_run(oracle, c, 0)
    tiny = np.float32(2.0 ** -126)
    assert np.isfinite(y).all() and np.any((y != 0) & (np.abs(y) < tiny)) and y[-1] == 0
    assert {int(fc.oracle_run(oracle, c, ch).view(np.uint32)[-1]) for ch in (0, 1)} <= {0, 0x80000000}


# ---- the host-only functions --------------------------------------------------------------------------------------------
def k0_formula(hq):
    s, k = 0, 0
    for v in np.asarray(hq, np.int64):
        s += abs(int(v))
        if s > 32767:
            break
        k += 1
    return k


def test_clamp_free_taps(capi, oracle):
    from oracle import bindings
    sums = {}
    for name in bindings.TAP_SETS:
        h, hq = oracle.taps_f32(name), oracle.taps_q15(name)
        assert capi.filter_clamp_free_taps(h) == k0_formula(hq) == fm.clamp_free_taps(hq), name
        sums[name] = (k0_formula(hq), len(hq))
    assert sums["wbfm_d1"] == (8, 8) and sums["am_s1"][0] == sums["am_s1"][1]              # clamp-free throughout
    assert sums["audio40"][0] < 40 and sums["ssb_hilbert"][0] < sums["ssb_hilbert"][1]
    assert sums["ssb_delay"][0] == 15                       # the tap of -32768 at index 15 is one over the bound
    q = lambda *v: np.float32(v) / np.float32(32768)
    assert capi.filter_clamp_free_taps(q(16384, -16383)) == 2             # sum exactly 32767
    assert capi.filter_clamp_free_taps(q(16384, -16384)) == 1             # sum exactly 32768
    assert capi.filter_clamp_free_taps(q(16384, -16383, 0, 0, 1)) == 4
    assert capi.filter_clamp_free_taps([1.0]) == 0 and capi.filter_clamp_free_taps([-1.0]) == 0   # both quantise to -32768
    assert capi.filter_clamp_free_taps([0.0] * 1024) == 1024
    rng = np.random.default_rng(2)
    for _ in range(50):
        h = rng.uniform(-1, 1, int(rng.integers(1, 200))).astype(np.float32) * np.float32(rng.choice([0.01, 0.1, 1.0]))
        assert capi.filter_clamp_free_taps(h) == k0_formula(fm.quantize(h))


def test_tile_samples(capi):
    for kind in ("decimate_i16", "fir_i16", "fir_f32"):
        for L in range(1, 1025):
            for factor in (range(1, 65) if kind == "decimate_i16" else (1,)):
                if factor in (1, 2, 3, 64) or L in (1, 40, 1024):
                    assert capi.filter_tile_samples(kind, L, 0, factor) == fc.T_FIR * factor
        bad = [(0, 0, 1), (1025, 0, 1), (8, 1, 1), (8, 0, 0), (8, 0, 65 if kind == "decimate_i16" else 2)]
        for L, nd, factor in bad:
            assert capi.filter_tile_samples(kind, L, nd, factor) == 0, (kind, L, nd, factor)
    for nb in range(1, 65):
        for na in range(1, 65):
            assert capi.filter_tile_samples("iir_f32", nb, na, 1) == fc.T_IIR
    for nb, na, factor in [(0, 1, 1), (65, 1, 1), (1, 0, 1), (1, 65, 1), (2, 1, 2), (2, 1, 0)]:
        assert capi.filter_tile_samples("iir_f32", nb, na, factor) == 0
    assert capi.filter_tile_samples(-1, 8, 0, 1) == 0 and capi.filter_tile_samples(4, 8, 0, 1) == 0


def test_exports_and_kind_names(capi):
    for name in ("iqd_filter_create", "iqd_filter_destroy", "iqd_filter_reset", "iqd_filter_out_count", "iqd_filter_run",
                 "iqd_filter_run_device", "iqd_filter_tile_samples", "iqd_filter_clamp_free_taps"):
        assert name in capi.EXPORTS and getattr(capi._lib(), name)
    assert capi.Filter.KINDS == KIND_CODE


# ---- the code object ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def code_object():
    """iqd_filter.hip cross-compiled for gfx950 (device only, the library's flags): ({kernel: metadata}, {kernel: text})"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta, text = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "iqd_filter.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
               os.path.join(csrc, "iqd_filter.hip")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        src = open(asm).read()
        for blk in re.split(r"\n\s+- \.agpr_count:", src)[1:]:
            kernel = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[kernel] = {k: int(v) for k, v in re.findall(
                r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\d+)", blk)}
        for kernel in meta:
            text[kernel] = re.search(r"\n%s:[^\n]*\n(.*?)\n\s+s_endpgm" % re.escape(kernel), src, re.S).group(1)
    return meta, text


def short_name(k):
    m = re.match(r"_ZN3iqd\d+(\w+?)(?:I(\w+?)E)?(?:EvNS|ENS)", k)
    args = {"s": "i16", "f": "f32", None: ""}.get(m.group(2), m.group(2))
    if args and args.startswith("Li"):
        args = ",".join(re.findall(r"Li(\d+)E", m.group(2) + "E"))
    return m.group(1) + ("<%s>" % args if args else "")


# VGPRs per lane as built.  The FIR and history kernels run 256-lane workgroups; the IIRs run single waves and
# hold the next tile (16 x float4) in registers while they walk the current one.
VGPRS = {"filter_fir_kernel<i16>": 20, "filter_fir_kernel<f32>": 20, "filter_history_kernel<i16>": 11,
         "filter_history_kernel<f32>": 11, "filter_iir_kernel": 184, "filter_iir_small_kernel<1,1>": 152,
         "filter_iir_small_kernel<1,2>": 156, "filter_iir_small_kernel<2,1>": 154, "filter_iir_small_kernel<2,2>": 156,
         "filter_iir_small_kernel<3,1>": 154, "filter_iir_small_kernel<3,2>": 156}


def test_code_object(code_object):
    meta, text = code_object
    got = {short_name(k): m for k, m in meta.items()}
    small = ["filter_iir_small_kernel<%d,%d>" % (nb, na) for nb in (1, 2, 3) for na in (1, 2)]
    assert sorted(got) == sorted(["filter_fir_kernel<i16>", "filter_fir_kernel<f32>", "filter_history_kernel<i16>",
                                  "filter_history_kernel<f32>", "filter_iir_kernel"] + small), sorted(got)
    for k, m in got.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        # 256-lane workgroups (FIR, history): up to 64 VGPRs keep eight of them on a CU.  The IIR's workgroups are single
        # waves (up to 512 would run): up to 256 keeps two waves on every SIMD
        assert m["vgpr_count"] <= (256 if "iir" in k else 64), (k, m)
    # the counts as built
    assert {k: m["vgpr_count"] for k, m in got.items()} == VGPRS, {k: m["vgpr_count"] for k, m in got.items()}
    assert got["filter_iir_kernel"]["group_segment_fixed_size"] == 49152          # tile + both rings
    assert got["filter_iir_small_kernel<3,2>"]["group_segment_fixed_size"] == 64 * 65 * 4
    q15 = text[[k for k in meta if short_name(k) == "filter_fir_kernel<i16>"][0]]
    assert "v_dot2_i32_i16" in q15 and "v_med3_i32" in q15
    assert "s_load_dword" in q15                              # the taps come through the scalar cache
    f32 = text[[k for k in meta if short_name(k) == "filter_fir_kernel<f32>"][0]]
    assert "v_mul_f32" in f32 and "v_add_f32" in f32        # (its 64-bit index division may use fused ops; the IIRs have none)
    for k in meta:
        if "iir" in k:
            assert "v_fma_f32" not in text[k] and "v_fmac_f32" not in text[k], k


def test_isa_lint_of_the_filter_kernels():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_filter.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 11 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
