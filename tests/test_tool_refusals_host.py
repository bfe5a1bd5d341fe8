"""CPU tier: everything the four C-ABI tools (iqdemod_wide, _spectrum, _filter, _multi) say and leave behind before they touch a
device - exit status, stderr text, and the files under the output directory with their sizes - equal to
tests/golden/tool_refusals.json key for key.  The table is tests/tool_cases.py's; the golden file is what the tools gave before
they were folded onto csrc/iqd_tool.h and csrc/iqd_tool_chain.h.  The cases that reach iqd_create ("no usable HIP device",
with the empty files the tool had made by then) are held to the file only where there is no GPU."""
import json
import os
import subprocess
import sys

import pytest

from tests import tool_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tool_refusals.json")


@pytest.fixture(scope="module")
def tiers():
    """torch.cuda.is_available(), asked in a child process: torch brings its own HIP runtime, which finds no device in a
    process where an engine has opened it first (tools/chan_fuzz.py: compute_units)"""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[-1] in ("True", "False"), r.stderr[-2000:]
    return ("cpu",) if r.stdout.split()[-1] == "True" else ("cpu", "nodevice")


def test_every_refusal_is_the_recorded_one(tiers, tmp_path):
    with open(GOLDEN) as f:
        text = f.read()
    recorded = json.loads(text)
    assert sorted(recorded) == sorted(c.name for c in tc.CASES if c.tier in ("cpu", "nodevice"))
    want = {c.name: recorded[c.name] for c in tc.CASES if c.tier in tiers}
    got = tc.collect(tmp_path, tiers, hashes=False)
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    if "nodevice" in tiers:
        assert tc.dump(got) == text


def test_the_table_reaches_what_the_issue_names():
    """the recorded file holds each kind of refusal the tools have, so that a table that lost one does not pass unnoticed"""
    with open(GOLDEN) as f:
        recorded = json.load(f)
    said = "".join(v["stderr"] for v in recorded.values())
    for part in ("unknown argument", "edges= takes three widths", "modes=auto and measlog= need tracks=", "rate must be 256000 P / Q",
                 "format must be u8, s8 or s16", "format=s8 cannot be combined with survey=", "format=s16 cannot be combined with scan=",
                 "cannot be combined with a fractional rate: not built for signed", "agc must be off, lowpass or harris",
                 "agc= / rxgain= cannot be combined with scan=", "agc= / rxgain= cannot be combined with a fractional rate",
                 "agc= / rxgain= cannot be combined with format=s8|s16", "tracks= cannot be combined with scan=",
                 "tracks= cannot be combined with agc= / rxgain=", "tracks= cannot be combined with a fractional rate",
                 "tracks= cannot be combined with format=s8|s16", "survey= cannot be combined with scan=", "survey offset", " offset -1024000 Hz",
                 "to be a multiple of 64\n", "to be a multiple of 256, at most 32768", "iqdemod_wide: cannot open", "iqdemod_wide: cannot create",
                 "usage: iqdemod_wide in=cap.iq [decimation", "usage: iqdemod_wide in=cap.iq rate=2048000 tracks=S", "events= needs track= and measure=",
                 "measure= needs track=", "track= needs detect=", "detect= needs rate", "does not hold 64 int16 values", "cannot open the files\n",
                 "usage: iqdemod_spectrum", "no coefficients in", "cannot open the files of channel", "usage: iqdemod_filter", "usage: <TOOL> channels=N",
                 "iqdemod_wide: iqd_create: no usable HIP device", "iqdemod_spectrum: iqd_create: no usable HIP device",
                 "iqdemod_filter: iqd_create: no usable HIP device", "iqdemod_multi: no usable HIP device"):
        assert part in said, part
    left = recorded["wide.no device"]["files"]
    assert left == {"p_0.s16": 0, "p_1.s16": 0, "f.txt": 0, "g.txt": 0, "sv.txt": 0}       # made before iqd_create, and left behind
    assert "m.txt" not in recorded["wide.tracks no device"]["files"]                       # measlog= is made after it
