"""GPU tier: rtlsdrdiags_amd/bin/iqdemod_tones against the Python path on the same PCM - its lines from files of three channels
of different lengths, whatever the chunk is, and from stdin - and its usage text for arguments it cannot take."""
import os
import subprocess

import numpy as np
import pytest

from rtlsdrdiags_amd import capi, tones
from tests import tones_cases as tc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_tones")
L = 256
HZ = [697.0, 770.0, 1209.5, 1336.0]


def script(phasor, text, n_extra):
    """a frame of L samples per letter: a..d = one of HZ, - = silence; n_extra samples of an open frame behind"""
    incs = [tones.phase_inc(int(round(f * 1000)), 8000) for f in HZ]
    parts = [np.zeros(L, np.int64) if ch == "-" else tc.tone(phasor, incs["abcd".index(ch)], 9000, L) for ch in text]
    return np.concatenate(parts + [np.full(n_extra, 77, np.int64)]).astype("<i2")


def python_lines(eng, rows, **cfg):
    """the tool's lines from Tones.run on the whole input in one call"""
    n = max(len(r) for r in rows)
    pcm = np.zeros((len(rows), n), np.int16)
    for c, r in enumerate(rows):
        pcm[c, :len(r)] = r
    mhz = [int(round(f * 1000)) for f in HZ]
    t = tones.Tones(eng, len(rows), np.array([tones.phase_inc(f, 8000) for f in mhz], np.uint32), frame_len=L, **cfg)
    nf, frames, _ = t.run(pcm, n, np.array([len(r) for r in rows], np.uint32), want_power=False)
    t.close()
    out = []
    for c in range(len(rows)):
        tone = -1
        for k in range(int(nf[c])):
            r = frames[c, k]
            if r["flags"]:
                opened, closed = bool(r["flags"] & tones.F_OPENED), bool(r["flags"] & tones.F_CLOSED)
                named = int(r["tone"]) if opened else tone
                out.append("ch %d frame %d t %.3f %s tone %d %.3f p_best %d p_second %d energy %d"
                           % (c, k, (k + 1) * L / 8000, "SWITCHED" if opened and closed else "OPENED" if opened else "CLOSED", named,
                              mhz[named] / 1000.0, r["p_best"], r["p_second"], r["energy"]))
            tone = int(r["tone"])
    return out


def test_tool_against_the_python_path(tmp_path):
    phasor = capi.channelizer_phasor_table()
    rows = [script(phasor, "aa-bbbcc--d-dd", 100), script(phasor, "--dd", 0), script(phasor, "abababab", 255)]
    for c, r in enumerate(rows):
        r.tofile(str(tmp_path / ("pcm_%d.s16" % c)))
    eng = capi.Engine(n_channels=1)
    try:
        want = python_lines(eng, rows, ratio_q8=512, open=2, hold=1, min_power=1000)
        kinds = {l.split()[6] for l in want}
        assert kinds == {"OPENED", "CLOSED", "SWITCHED"} and {l.split()[1] for l in want} == {"0", "1"}, want   # channel 2 never opens
        args = [TOOL, "tones=" + ",".join("%g" % f for f in HZ), "frame=%d" % L, "minpower=1000", "channels=3", "in=" + str(tmp_path / "pcm_%d.s16")]
        for chunk in ("chunk=65536", "chunk=1000", "chunk=%d" % L):
            run = subprocess.run(args + [chunk], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
            assert run.returncode == 0 and run.stderr == "", run
            assert sorted(run.stdout.splitlines()) == sorted(want), chunk          # (the tool prints call by call)
        log = tmp_path / "tones.txt"
        run = subprocess.run(args + ["log=" + str(log)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert run.returncode == 0 and run.stdout == "" and log.read_text().splitlines() == want

        # stdin, one channel, the dtmf set's defaults: frame=256 ratio_q8=256 open=1 hold=0
        one = python_lines(eng, rows[:1], ratio_q8=256, open=1, hold=0, min_power=1000)
        run = subprocess.run([TOOL, "tones=" + ",".join("%g" % f for f in HZ), "frame=256", "ratio_q8=256", "open=1", "hold=0", "minpower=1000"],
                             input=rows[0].tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert run.returncode == 0 and run.stdout.decode().splitlines() == one and len(one) > len([l for l in want if l.startswith("ch 0")])
    finally:
        eng.close()


@pytest.mark.parametrize("args", [[], ["set=morse"], ["set=ctcss", "tones=100"], ["set=ctcss", "in=x_%d.s16"], ["set=ctcss", "channels=2"],
                                  ["tones=" + ",".join(["100"] * 65)], ["set=ctcss", "chunk=0"]])
def test_tool_usage(args):
    run = subprocess.run([TOOL] + args, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert run.returncode == 1 and run.stdout == "" and run.stderr.startswith("usage: iqdemod_tones set=ctcss|dtmf | tones=f1,f2,...")


def test_tool_refusals():
    run = subprocess.run([TOOL, "set=ctcss", "frame=100"], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=60)
    assert run.returncode == 1 and "iqd_tones_create" in run.stderr and "frame_len" in run.stderr
    run = subprocess.run([TOOL, "tones=5000", "rate=8000"], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=60)
    assert run.returncode == 1 and "needs a rate above" in run.stderr
    run = subprocess.run([TOOL, "set=ctcss", "bogus=1"], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=60)
    assert run.returncode == 1 and run.stderr == "iqdemod_tones: unknown argument bogus=1\n"
