"""GPU tier: rtlsdrdiags_amd/bin/iqdemod_fsk against the Python path on the same PCM - its lines from files of three channels of
different lengths, whatever the chunk is, and from stdin; the AX.25 addresses it names; its bit dump; and its usage text and
unknown-argument message."""
import os
import subprocess

import numpy as np
import pytest

from rtlsdrdiags_amd import capi, fsk
from tests import fsk_model as fm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "rtlsdrdiags_amd", "bin", "iqdemod_fsk")
USAGE = "usage: iqdemod_fsk set=afsk1200 | mark=HZ space=HZ baud=BD"


def address(call, ssid, last=False):
    return bytes(ord(ch) << 1 for ch in call.ljust(6)) + bytes([0x60 | ssid << 1 | int(last)])


UI = address("APRS", 0) + address("N0CALL", 7) + address("WIDE1", 1) + address("WIDE2", 2, last=True) + b"\x03\xf0!4903.50N/07201.75W-test"
PLAIN = bytes(range(200, 230))                       # no addresses: 0xc9 has its lowest bit set


def addresses(p):
    """the tool's rule in Python: 'SRC>DST[,PATH] ' or ''"""
    names = []
    for at in range(0, len(p) - 6, 7):
        if len(names) == 10:
            break
        if any(b & 1 for b in p[at:at + 6]):
            return ""
        s = "".join(chr(b >> 1) for b in p[at:at + 6])
        if not all(ch.isdigit() or "A" <= ch <= "Z" or ch == " " for ch in s):
            return ""
        s = s.rstrip(" ")
        if not s or " " in s:
            return ""
        ssid = p[at + 6] >> 1 & 15
        names.append(s + ("-%d" % ssid if ssid else ""))
        if p[at + 6] & 1:
            return "" if len(names) < 2 else names[1] + ">" + ",".join([names[0]] + names[2:]) + " "
    return ""


def pcm_of(phasor, payloads, lead=0, amp=9000):
    cfg = fm.afsk1200(8000)
    bits = [0, 0, 0] + fm.hdlc_bits(payloads, 4, 1, 2)
    x = fm.afsk(fm.nrzi_levels(bits), phasor, cfg["mark_inc"], cfg["space_inc"], cfg["baud_inc"], amp)
    return np.concatenate([np.zeros(lead, np.int64), x, np.zeros(40, np.int64)]).astype("<i2")


def python_lines(eng, rows, **over):
    """the tool's lines and bit texts from Fsk.run on the whole input in one call"""
    n = max(len(r) for r in rows)
    pcm = np.zeros((len(rows), n), np.int16)
    for c, r in enumerate(rows):
        pcm[c, :len(r)] = r
    t = fsk.Fsk(eng, len(rows), **dict(fsk.afsk1200(8000), **over))
    nb, bits, nf, frames, data = t.run(pcm, n, np.array([len(r) for r in rows], np.uint32))
    t.close()
    out = []
    for c, end, payload, _ in fsk.frames_of(nf, frames, data):
        out.append("ch %d end %d t %.4f len %d %s%s" % (c, end, end / 8000, len(payload), addresses(payload), payload.hex()))
    texts = ["".join(str(int(bits[c, i // 32]) >> (i % 32) & 1) for i in range(int(nb[c]))) for c in range(len(rows))]
    return out, texts


def test_tool_against_the_python_path(tmp_path):
    phasor = capi.channelizer_phasor_table()
    rows = [pcm_of(phasor, [UI, PLAIN]), pcm_of(phasor, [PLAIN], lead=777), pcm_of(phasor, [UI[:20], UI], lead=13, amp=3000)]
    for c, r in enumerate(rows):
        r.tofile(str(tmp_path / ("pcm_%d.s16" % c)))
    eng = capi.Engine(n_channels=1)
    try:
        want, texts = python_lines(eng, rows)
        assert len(want) == 5 and sum(" N0CALL-7>APRS,WIDE1-1,WIDE2-2 " in l for l in want) == 2, want
        assert sum(">" in l for l in want) == 2 and [l.split()[1] for l in want] == ["0", "0", "1", "2", "2"]
        args = [TOOL, "set=afsk1200", "channels=3", "in=" + str(tmp_path / "pcm_%d.s16")]
        for chunk in ("chunk=65536", "chunk=1000", "chunk=64"):
            run = subprocess.run(args + [chunk], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
            assert run.returncode == 0 and run.stderr == "", run
            assert sorted(run.stdout.splitlines()) == sorted(want), chunk          # (the tool prints call by call)
        log = tmp_path / "frames.txt"
        run = subprocess.run(args + ["log=" + str(log), "bits=" + str(tmp_path / "bits_%d.txt"), "chunk=999"], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, timeout=120)
        assert run.returncode == 0 and run.stdout == "" and sorted(log.read_text().splitlines()) == sorted(want)
        assert [(tmp_path / ("bits_%d.txt" % c)).read_text() for c in range(3)] == texts and min(len(t) for t in texts) > 300

        # stdin, one channel, every argument spelled out and a longer min_len: the short frame goes
        one, _ = python_lines(eng, rows[2:], min_len=30)
        run = subprocess.run([TOOL, "mark=1200", "space=2200", "baud=1200", "rate=8000", "corr=8", "loop=3", "nrzi=1", "minlen=30", "maxlen=512"],
                             input=rows[2].tobytes(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert run.returncode == 0 and run.stdout.decode().splitlines() == one and len(one) == 1
    finally:
        eng.close()


@pytest.mark.parametrize("args", [[], ["set=pocsag"], ["mark=1200", "space=2200"], ["set=afsk1200", "in=x_%d.s16"], ["set=afsk1200", "channels=2"],
                                  ["set=afsk1200", "nrzi=2"], ["set=afsk1200", "chunk=0"]])
def test_tool_usage(args):
    run = subprocess.run([TOOL] + args, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert run.returncode == 1 and run.stdout == "" and run.stderr.startswith(USAGE)


def test_tool_refusals():
    run = subprocess.run([TOOL, "set=afsk1200", "corr=100"], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=60)
    assert run.returncode == 1 and "iqd_fsk_create" in run.stderr and "corr_len" in run.stderr
    run = subprocess.run([TOOL, "set=afsk1200", "rate=4000"], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=60)
    assert run.returncode == 1 and "needs a rate above" in run.stderr
    run = subprocess.run([TOOL, "set=afsk1200", "bogus=1"], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=60)
    assert run.returncode == 1 and run.stderr == "iqdemod_fsk: unknown argument bogus=1\n"
