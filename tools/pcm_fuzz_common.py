"""What the fuzzers of the PCM add-ons share (tools/tones_fuzz.py, tools/fsk_fuzz.py): the case generator's seed, the device
buffers, the rows' upload, a case's run against its model, and the command line.  Each fuzzer keeps its own draw(): the order
of its random draws names its cases."""
import argparse
import time

import numpy as np

from rtlsdrdiags_amd import capi


def case_rng(seed, index):
    return np.random.default_rng([int(seed), int(index)])


def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


class Buffers:
    """device arrays that grow and are reused from call to call uncleared"""

    def __init__(self, eng):
        self.eng, self.ptr, self.cap = eng, {}, {}

    def get(self, name, nbytes):
        if self.cap.get(name, 0) < nbytes:
            if name in self.ptr:
                self.eng.dev_free(self.ptr[name])
            self.cap[name] = 2 * nbytes + 64
            self.ptr[name] = self.eng.dev_alloc(self.cap[name])
        return self.ptr[name]

    def close(self):
        for p in self.ptr.values():
            self.eng.dev_free(p)
        self.ptr, self.cap = {}, {}


def upload_rows(eng, bufs, pcm, count):
    """(pcm_dev, count_dev or 0): the rows from 2 bytes behind an aligned address on"""
    p_pcm = bufs.get("pcm", pcm.nbytes + 16) + 2
    eng.dev_upload(p_pcm - 2, np.concatenate([np.zeros(1, np.int16), pcm.reshape(-1)]))
    p_cnt = 0
    if count is not None:
        p_cnt = bufs.get("count", pcm.shape[0] * 4)
        eng.dev_upload(p_cnt, count)
    return p_pcm, p_cnt


# how one array of a call's result is held against the model's: None, or what differs
def equal(got, want):
    return None if np.array_equal(got, want) else (got, want)


def records(got, want):
    return None if got.tobytes() == want.tobytes() else [k for k in want.dtype.names if not np.array_equal(got[k], want[k])]


def run_case(case, model, make, run_device, option, compares, gpu):
    """The model's results, step by step.  With gpu, make() is the library's object, and every array of every step - compares: a
    (name, compare) each, compare None for the optional one, which is there iff the step asks for it; option: run()'s keyword
    for it - and three channels' states are held against the model's."""
    who = "seed %d case %d" % (case["seed"], case["index"])
    t = make() if gpu else None
    out = []
    try:
        for i, s in enumerate(case["steps"]):
            if s[0] == "reset":
                model.reset()
                if gpu:
                    t.reset()
                continue
            _, pcm, n, count, given, form = s
            want = model.run(pcm, n, count)
            out.append(want)
            if not gpu:
                continue
            got = t.run(pcm, n, count, **{option: given}) if form == "host" else run_device(t, pcm, n, count, given)
            assert len(got) == len(want) == len(compares), (who, i, len(got), len(want))
            for (name, compare), g, w in zip(compares, got, want):
                if compare is None:
                    assert (g is None) == (not given), (who, i, name)
                bad = None if g is None else (compare or equal)(g, w)
                assert bad is None, (who, i, name, bad)
        if gpu:
            for c in sorted({0, case["C"] // 2, case["C"] - 1}):
                assert t.state(c) == model.state(c), (who, "state", c, t.state(c), model.state(c))
    finally:
        if t is not None:
            t.close()
    return out


def main(name, slice_, draw, run_case_):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=slice_[0])
    ap.add_argument("--cases", type=int, default=slice_[1])
    ap.add_argument("--case", type=int, default=None)
    a = ap.parse_args()
    phasor = capi.channelizer_phasor_table()
    eng = capi.Engine(n_channels=1)
    bufs = Buffers(eng)
    t0 = time.time()
    todo = [a.case] if a.case is not None else range(a.cases)
    for i in todo:
        run_case_(draw(a.seed, i, phasor), phasor, eng, bufs)
    bufs.close()
    eng.close()
    print("%s: seed %d, %d case(s) identical to the model in %.1f s" % (name, a.seed, len(todo), time.time() - t0))
