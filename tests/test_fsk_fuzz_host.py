"""CPU tier: the fixed slice of tools/fsk_fuzz.py that tests/test_gpu_fsk_fuzz.py runs, drawn and run through the model alone -
the draws stay inside the header's ranges (the model's results exist), name the same case twice, and between them reach what
the fuzzer is there for."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fsk_fuzz as ff                                  # noqa: E402
from rtlsdrdiags_amd import capi                       # noqa: E402


def test_the_slice_reaches_what_it_is_for():
    phasor = capi.channelizer_phasor_table()
    seed, cases = ff.SLICE
    seen = dict(forms=set(), reset=0, counted=0, no_bits=0, short=0, frames=0, two_in_a_call=0, tail=0, bad_fcs=0, bits=0, W=set(), C=set(),
                n=set(), shift=set(), flags=set(), windows=0, carried=0)
    for i in range(cases):
        case = ff.draw(seed, i, phasor)
        cfg = case["cfg"]
        assert 2 <= cfg["corr_len"] <= 64 and 2 ** 20 <= cfg["baud_inc"] < 2 ** 31 and 1 <= cfg["loop_shift"] <= 8 and cfg["flags"] in (0, 1)
        assert 3 <= cfg["min_len"] <= cfg["max_len"] <= 1024 and (case["window"] is None or np.abs(case["window"].astype(np.int64)).max() <= 32512)
        seen["W"].add(cfg["corr_len"]); seen["C"].add(case["C"]); seen["shift"].add(cfg["loop_shift"]); seen["flags"].add(cfg["flags"])
        seen["windows"] += case["window"] is not None
        runs = [s for s in case["steps"] if s[0] == "run"]
        assert all(s[2] <= s[1].shape[1] for s in runs)
        seen["n"] |= {s[2] for s in runs}
        seen["reset"] += any(s[0] == "reset" for s in case["steps"])
        seen["counted"] += any(s[3] is not None for s in runs)
        seen["no_bits"] += any(not s[4] for s in runs)
        seen["forms"] |= {s[5] for s in runs}
        seen["short"] += sum(0 < s[2] < cfg["corr_len"] for s in runs)
        out, states = ff.run_case(case, phasor, gpu=False)
        for k, (nb, bits, nf, frames, data) in enumerate(out):
            seen["bits"] += int(nb.sum())
            seen["frames"] += int(nf.sum())
            seen["two_in_a_call"] += int((nf >= 2).sum())
            seen["tail"] += bool(len(nf) > 1 and nf.min() < frames.shape[1] and nf.max() > 0)
            seen["carried"] += int(k > 0 and nf.sum() > 0)
        seen["bad_fcs"] += sum(s["bad_fcs"] for s in states)
    assert seen["forms"] == {"host", "device"} and seen["flags"] == {0, 1} and seen["shift"] == set(range(1, 9))
    assert seen["W"] >= set(ff.W_EDGES) and seen["C"] >= set(ff.C_EDGES) and seen["n"] >= set(ff.N_EDGES)
    assert min(seen[k] for k in ("reset", "counted", "no_bits", "short", "two_in_a_call", "tail", "bad_fcs", "windows", "carried")) >= 10, seen
    assert seen["frames"] > 200 and seen["bits"] > 100000, seen
    again = ff.draw(seed, 17, phasor)
    first = ff.draw(seed, 17, phasor)
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(again["steps"], first["steps"]) if a[0] == "run") and again["cfg"] == first["cfg"]
