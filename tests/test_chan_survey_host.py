"""CPU tier: the channelizer's band survey (include/iqdemod.h: "Band survey") without a GPU - its numpy model
(tests/chan_survey_model.py) against the oracle's detector, the mutation proof of the GPU test's inputs
(tests/chan_survey_cases.py), iqd_magnitude_dbfs against the golden table and the oracle, and the cross-compiled kernels'
code object."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import chan_survey_cases as sc
from tests import chan_survey_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from rtlsdrdiags_amd import capi as c
    return c


@pytest.fixture(scope="module")
def P(capi):
    return capi.channelizer_phasor_table()


def test_magnitude_dbfs_is_the_squelch_table(capi, golden, oracle):
    got = np.array([capi.magnitude_dbfs(m) for m in range(300)], np.int64)
    assert np.array_equal(got, golden["primitives"]["dbfs_0_299"].astype(np.int64))
    assert np.array_equal(got, np.array([oracle.dbfs(m) for m in range(300)], np.int64))
    assert capi.magnitude_dbfs(2 ** 32 - 1) == capi.magnitude_dbfs(127)


def test_model_detector_is_the_oracles(oracle):
    """the numpy per-sample magnitude (the defects are switched on in it) sums to the oracle's block_magnitude, rails
    included"""
    rng = np.random.default_rng(1)
    for n in (32, 64, 2560):
        u = rng.integers(0, 256, (1, 1, 2 * n), dtype=np.uint8)
        u[0, 0, :8] = [0, 0, 255, 255, 0, 255, 128, 0]
        want = oracle.block_magnitude((u[0, 0] ^ 0x80).view(np.int8))
        assert sm.reduce(u, n)[0, 0, 0] == want == sm.reduce(u, n, oracle=oracle)[0, 0, 0]
    assert sm.sample_magnitude(np.array([0, 0], np.uint8))[0] == 192


def blind(c):
    """the defects a case cannot see by construction"""
    out = set()
    if c.n_out == c.block_out:
        out |= {"boundary_late", "div_call"}       # one block: no boundary, and the call's outputs are the block's
    if c.pre == 0:
        out.add("zero_history")                    # the first call: the history is zero
    if c.n_src == 1:
        out.add("source_0")
    return out


def test_every_gpu_input_sees_every_defect(capi, P, oracle):
    """The model with one defect switched on must change some expected entry of each case the GPU test runs, except where
    the case cannot see the defect by construction; and every defect is seen at an integer and at a fractional rate."""
    seen = {1: set(), 2: set()}
    for c in sc.cases(capi):
        assert c.window == 1024                    # ("three windows", "tail" in the case list rest on it)
        rws = sm.rows(c.wide, c.h, c.M, c.Q, c.inc, c.shift, P, c.m_first, c.n_out)
        assert (rws == 0).any() and (rws == 255).any(), c              # 0x00 (|-128|) and 0xFF in the virtual rows
        want = sm.reduce(rws, c.block_out, c.window, oracle)
        assert np.array_equal(want, sm.reduce(rws, c.block_out, c.window)), c
        assert want.shape == (c.n_src, c.n_out // c.block_out, c.n_pts) and want.max() <= 192
        unseen = set()
        for mu in sm.MUTANTS:
            r = sm.rows(c.wide, c.h, c.M, c.Q, c.inc, c.shift, P, c.m_first, c.n_out, mu) if mu in sm.ROW_MUTANTS else rws
            if np.array_equal(sm.reduce(r, c.block_out, c.window, oracle, mu), want):
                unseen.add(mu)
            else:
                seen[min(c.Q, 2)].add(mu)
        assert unseen == blind(c), (c, unseen)
    assert seen[1] == set(sm.MUTANTS) and seen[2] == set(sm.MUTANTS)


def test_survey_is_what_the_squelch_reports(capi, P, oracle):
    """entry (s, b, p) is the magnitude the oracle's chain reports for block b of the channel's row"""
    c = [c for c in sc.cases(capi) if c.name == "M8-1pt-1blk"][0]
    row = sm.rows(c.wide, c.h, c.M, c.Q, c.inc, c.shift, P)[0, 0]
    ch = oracle.chain()
    _, mag, _ = ch.accept_stream(row)
    want = sm.survey(c.wide, c.h, c.M, c.Q, c.inc, c.shift, P, c.block_out, oracle=oracle)
    assert len(mag) == 1 and int(mag[0]) == int(want[0, 0, 0])


@pytest.fixture(scope="module")
def code_object():
    """iqd_chan_survey.hip cross-compiled for gfx950 (device only, the library's flags): {kernel: metadata}"""
    csrc = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc")
    meta = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "iqd_chan_survey.s")
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-strict-aliasing",
               "-I" + csrc, "-I" + os.path.join(ROOT, "include"), "-S", "--cuda-device-only", "-o", asm,
               os.path.join(csrc, "iqd_chan_survey.hip")]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        for blk in re.split(r"\n\s+- \.agpr_count:", open(asm).read())[1:]:
            kernel = re.search(r"\.name:\s+(\S+)", blk).group(1)
            meta[kernel] = {k: int(v) for k, v in re.findall(
                r"\.(vgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", blk)}
    return meta


def test_code_object_has_no_private_segment_and_keeps_full_occupancy(code_object):
    survey = [k for k in code_object if "chz_survey_kernel" in k]
    assert len(survey) == 5 and len(code_object) == 6, sorted(code_object)    # Q = 1 (registers, L2), 2, 4, 8; the divider
    for k, m in code_object.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["vgpr_count"] <= 128, (k, m)                                 # 512 threads per workgroup
    got = {re.search(r"ILi(\d)ELi(\d)E", k).groups(): code_object[k]["vgpr_count"] for k in survey}
    assert got == {("1", "8"): 126, ("1", "0"): 70, ("2", "0"): 81, ("4", "0"): 84, ("8", "0"): 80}, got


def test_isa_lint_of_the_survey_kernels():
    src = os.path.join(ROOT, "rtlsdrdiags_amd", "csrc", "iqd_chan_survey.hip")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_lint.py"), src], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-4000:]
    last = r.stdout.strip().splitlines()[-1]
    assert " 6 kernels" in last and "0 finding(s)" in last and "0 kernel(s) with scratch" in last, last
