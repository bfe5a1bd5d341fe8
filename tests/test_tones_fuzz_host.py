"""CPU tier: the fixed slice of tools/tones_fuzz.py that tests/test_gpu_tones_fuzz.py runs, drawn and run through the model
alone - the draws stay inside the header's ranges (the model's results exist), name the same case twice, and between them reach
what the fuzzer is there for."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tones_fuzz as tf                                # noqa: E402
from rtlsdrdiags_amd import capi                       # noqa: E402
from tests import tones_model as tm                    # noqa: E402


def test_the_slice_reaches_what_it_is_for():
    phasor = capi.channelizer_phasor_table()
    seed, cases = tf.SLICE
    seen = dict(flags=set(), forms=set(), reset=0, counted=0, no_power=0, straddle=0, tail=0, hits=0, misses=0, ties=0, L=set(), T=set(), C=set())
    for i in range(cases):
        case = tf.draw(seed, i, phasor)
        assert 32 <= case["L"] <= 8192 and case["L"] % 32 == 0 and 1 <= len(case["incs"]) <= 64 and 256 <= case["cfg"]["ratio_q8"] <= 65535
        assert 0 <= case["cfg"]["energy_q8"] <= 2 ** 20 and 1 <= case["cfg"]["open"] <= 255 and 0 <= case["cfg"]["hold"] <= 255
        seen["L"].add(case["L"]); seen["T"].add(len(case["incs"])); seen["C"].add(case["C"])
        runs = [s for s in case["steps"] if s[0] == "run"]
        assert all(s[2] <= s[1].shape[1] for s in runs)
        seen["reset"] += any(s[0] == "reset" for s in case["steps"])
        seen["counted"] += any(s[3] is not None for s in runs)
        seen["no_power"] += any(not s[4] for s in runs)
        seen["forms"] |= {s[5] for s in runs}
        seen["straddle"] += sum(0 < s[2] < case["L"] for s in runs) >= 2
        for nf, frames, power in tf.run_case(case, phasor, gpu=False):
            seen["flags"] |= {int(f) for f in np.unique(frames["flags"])}
            seen["tail"] += bool(len(nf) > 1 and nf.min() < frames.shape[1] and nf.max() > 0)
            done = [frames[c, :int(nf[c])] for c in range(len(nf))]
            seen["hits"] += sum(int((d["tone"] >= 0).sum()) for d in done)
            seen["misses"] += sum(int((d["tone"] < 0).sum()) for d in done)
            seen["ties"] += sum(int(((d["p_best"] == d["p_second"]) & (d["p_best"] > 0)).sum()) for d in done)
    assert seen["flags"] == {0, 1, 2, 3} and seen["forms"] == {"host", "device"}
    assert seen["L"] >= set(tf.L_EDGES) and seen["T"] >= set(tf.T_EDGES) and seen["C"] >= set(tf.C_EDGES)
    assert min(seen[k] for k in ("reset", "counted", "no_power", "straddle", "tail", "ties")) >= 10, seen
    assert seen["hits"] > 500 and seen["misses"] > 500, seen                       # frames with and without a tone in force
    again = tf.draw(seed, 17, phasor)
    first = tf.draw(seed, 17, phasor)
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(again["steps"], first["steps"]) if a[0] == "run") and again["incs"] == first["incs"]
