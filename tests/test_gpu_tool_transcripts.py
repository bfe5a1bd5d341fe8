"""GPU (MI355X): the four C-ABI tools (iqdemod_wide, _spectrum, _filter, _multi) over a few engine blocks each - exit status,
stderr, and the length and sha256 of every file they write - equal to tests/golden/tool_transcripts.json key for key.  The
table is tests/tool_cases.py's (every capture ends inside a call); the golden file is what the tools gave before they were
folded onto csrc/iqd_tool.h and csrc/iqd_tool_chain.h.  The engine is bit-exact, so a hash is a fair fixture; what the bytes
mean is held by the per-feature tool tests against the Python path."""
import json
import os

import pytest

from tests import tool_cases as tc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tool_transcripts.json")


def test_every_transcript_is_the_recorded_one(tmp_path):
    with open(GOLDEN) as f:
        text = f.read()
    want = json.loads(text)
    got = tc.collect(tmp_path, ("gpu",), hashes=True)
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert tc.dump(got) == text


def test_the_recorded_runs_are_not_empty():
    """the golden file's own content: the band chain cases found tracks, measured them and logged events, the notices printed"""
    with open(GOLDEN) as f:
        want = json.load(f)
    assert len(want) == len([c for c in tc.CASES if c.tier == "gpu"])
    chain = want["spectrum.band chain"]
    assert chain["status"] == 0 and "runs past maxdet not written" in chain["stderr"] and "bytes after the last whole block dropped" in chain["stderr"]
    assert all(chain["files"][n][0] > 0 for n in ("pw.u32", "log.txt", "runs.txt", "tracks.txt", "meas.txt", "events.txt"))
    auto = want["wide.tracks modes=auto"]
    assert auto["status"] == 0 and "300 trailing bytes" in auto["stderr"] and all(v[0] > 0 for v in auto["files"].values())
    assert "is not surveyed" in want["wide.survey, short block not surveyed"]["stderr"]
    assert sorted(want["wide.survey alone"]["files"]) == ["sv.txt"]
    assert [want[k]["status"] for k in ("wide.library refuses gains=9", "spectrum.library refuses bins=100")] == [1, 1]
