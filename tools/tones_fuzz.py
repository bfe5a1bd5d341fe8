"""Diagnostic: randomized tone-bank runs on an MI355X, every array bit for bit against the model written from the header
(include/iqdemod_tones.h; tests/tones_model.py).

    python tools/tones_fuzz.py [--seed S] [--cases N]        a campaign
    python tools/tones_fuzz.py --seed S --case I             one case again

Case I of seed S is drawn from numpy's default_rng([S, I]) and from nothing else, so (seed, index) names a case on every
machine.  A case is drawn without a GPU (draw) and then run (run_case; gpu=False runs the model alone).  About every second
parameter comes from a list of edges, the rest at random, all inside the ranges the header documents.  Refusals are not fuzzed.

  bank      L around the K-chunk (32 .. 256, sometimes 1024), T around the MFMA tile's 8 tones, channels around the
            workgroup's 16; increments at random, on bins of L, duplicated; the default window, a random one, +-32767
  thresholds ratio_q8 over its whole range, energy_q8 and min_power zero or not, open 1 .. 4, hold 0 .. 3
  samples   per channel and frame: noise, one of the tones in noise, two tones, silence, +-32767 alternating, -32768
  calls     one to five, n from {0, 1, L - 1, L, L + 1, 3 L + 5} or at random, row_stride >= n, rows 2-byte aligned only;
            counts (0 and above n among them) or none; power or none; the host form or the device form; a reset in between"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                     # noqa: E402
from rtlsdrdiags_amd import capi, tones                # noqa: E402
from tests import tones_model as tm                    # noqa: E402

L_EDGES = (32, 64, 96, 128, 160, 256)
T_EDGES = (1, 2, 7, 8, 9, 15, 16, 17, 33, 64)
C_EDGES = (1, 2, 15, 16, 17, 33)
SLICE = (9401, 300)            # (seed, cases): tests/test_gpu_tones_fuzz.py's


def case_rng(seed, index):
    return np.random.default_rng([int(seed), int(index)])


def pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def draw(seed, index, phasor):
    """dict(cfg for tm.Model / tones.Tones, steps: ("reset",) or ("run", pcm, n, count, want_power, form))"""
    rng = case_rng(seed, index)
    L = 1024 if rng.random() < 0.04 else pick(rng, L_EDGES)
    T = pick(rng, T_EDGES) if rng.random() < 0.6 else int(rng.integers(1, 65))
    C = pick(rng, C_EDGES) if rng.random() < 0.6 else int(rng.integers(1, 40))
    if L == 1024:
        C = min(C, 4)
    incs = []
    for t in range(T):
        u = rng.random()
        incs.append(incs[int(rng.integers(len(incs)))] if incs and u < 0.15 else
                    (int(rng.integers(0, L)) << 32) // L if u < 0.6 else int(rng.integers(0, 2 ** 32)))
    u = rng.random()
    window = (None if u < 0.4 else rng.integers(-32767, 32768, L).astype(np.int16) if u < 0.8 else
              np.full(L, pick(rng, (32767, -32767)), np.int16))
    cfg = dict(min_power=0 if rng.random() < 0.5 else int(2 ** rng.uniform(0, 56)),
               ratio_q8=pick(rng, (256, 257, 512, 65535)) if rng.random() < 0.5 else int(2 ** rng.uniform(8, 16)),
               energy_q8=0 if rng.random() < 0.5 else int(2 ** rng.uniform(0, 20)), open=int(rng.integers(1, 5)), hold=int(rng.integers(0, 4)))
    cfg["ratio_q8"] = min(max(cfg["ratio_q8"], 256), 65535)
    steps = []
    for _ in range(int(rng.integers(1, 6))):
        if steps and rng.random() < 0.15:
            steps.append(("reset",))
        n = pick(rng, (0, 1, L - 1, L, L + 1, 3 * L + 5)) if rng.random() < 0.6 else int(rng.integers(0, 4 * L))
        stride = n + int(pick(rng, (0, 1, 3, 8)))
        pcm = rng.integers(-32768, 32768, (C, max(stride, 1))).astype(np.int16)       # (what lies behind n is never read)
        k = np.arange(n, dtype=np.uint64)
        for c in range(C):
            for a in range(0, n, L):                           # the kinds change every L samples: not on the frames' grid
                b, u = min(a + L, n), rng.random()
                amp = int(2 ** rng.uniform(4, 14))
                seg = rng.integers(-amp // 8 - 1, amp // 8 + 2, b - a)
                if u < 0.45:
                    for d in ([pick(rng, incs)] if u < 0.35 else [pick(rng, incs), pick(rng, incs)]):
                        i = (((k[a:b] * np.uint64(d)) & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.int64)
                        seg = seg + ((amp * phasor[i, 0].astype(np.int64)) >> 15)
                elif u < 0.6:
                    seg = np.zeros(b - a, np.int64)
                elif u < 0.7:
                    seg = np.where(np.arange(b - a) % 2 == 0, 32767, -32767)
                elif u < 0.75:
                    seg = np.full(b - a, -32768)
                pcm[c, a:b] = np.clip(seg, -32768, 32767)
        count = None
        if rng.random() < 0.4:
            count = rng.integers(0, n + 3, C).astype(np.uint32)
            count[int(rng.integers(C))] = pick(rng, (0, n, n + 7))
        steps.append(("run", pcm, n, count, rng.random() < 0.7, "host" if rng.random() < 0.3 else "device"))
    return dict(seed=seed, index=index, C=C, L=L, incs=incs, window=window, cfg=cfg, steps=steps)


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


def run_device(eng, bufs, t, pcm, n, count, want_power):
    C, stride = pcm.shape
    F, T = t.max_frames(n), t.n_tones
    p_pcm = bufs.get("pcm", pcm.nbytes + 16) + 2                    # rows from 2 bytes behind an aligned address on
    eng.dev_upload(p_pcm - 2, np.concatenate([np.zeros(1, np.int16), pcm.reshape(-1)]))
    p_cnt = 0
    if count is not None:
        p_cnt = bufs.get("count", C * 4)
        eng.dev_upload(p_cnt, count)
    p_nf, p_fr, p_pw = bufs.get("nf", C * 4), bufs.get("frames", C * F * 40 + 16), bufs.get("power", C * F * T * 8 + 16)
    t.run_device(p_pcm, stride, n, p_nf, p_fr, power_dev=p_pw if want_power else 0, count_dev=p_cnt)
    eng.synchronize()
    nf = eng.dev_download(p_nf, C * 4, np.uint32)
    frames, power = np.zeros((C, F), tones.TONES_FRAME), (np.zeros((C, F, T), np.uint64) if want_power else None)
    if F:
        frames = eng.dev_download(p_fr, C * F * 40).view(tones.TONES_FRAME).reshape(C, F)
        if want_power:
            power = eng.dev_download(p_pw, C * F * T * 8, np.uint64).reshape(C, F, T)
    return nf, frames, power


def run_case(case, phasor, eng=None, bufs=None, gpu=True):
    """the model's results; with gpu, the library's held against them (AssertionError names the case and the step)"""
    who = "seed %d case %d" % (case["seed"], case["index"])
    m = tm.Model(case["C"], case["L"], case["incs"], phasor, window=case["window"], **case["cfg"])
    t = tones.Tones(eng, case["C"], np.array(case["incs"], np.uint32), frame_len=case["L"], window=case["window"], **case["cfg"]) if gpu else None
    out = []
    try:
        for i, s in enumerate(case["steps"]):
            if s[0] == "reset":
                m.reset()
                if gpu:
                    t.reset()
                continue
            _, pcm, n, count, want_power, form = s
            want = m.run(pcm, n, count)
            out.append(want)
            if not gpu:
                continue
            got = t.run(pcm, n, count, want_power=want_power) if form == "host" else run_device(eng, bufs, t, pcm, n, count, want_power)
            assert np.array_equal(got[0], want[0]), (who, i, "n_frames", got[0], want[0])
            assert got[1].tobytes() == want[1].tobytes(), (who, i, "frames", [k for k in tm.FRAME.names if not np.array_equal(got[1][k], want[1][k])])
            assert (got[2] is None) == (not want_power) and (got[2] is None or np.array_equal(got[2], want[2])), (who, i, "power")
        if gpu:
            for c in sorted({0, case["C"] // 2, case["C"] - 1}):
                assert t.state(c) == m.state(c), (who, "state", c, t.state(c), m.state(c))
    finally:
        if t is not None:
            t.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=SLICE[0])
    ap.add_argument("--cases", type=int, default=SLICE[1])
    ap.add_argument("--case", type=int, default=None)
    a = ap.parse_args()
    phasor = capi.channelizer_phasor_table()
    eng = capi.Engine(n_channels=1)
    bufs = Buffers(eng)
    t0 = time.time()
    todo = [a.case] if a.case is not None else range(a.cases)
    for i in todo:
        run_case(draw(a.seed, i, phasor), phasor, eng, bufs)
    bufs.close()
    eng.close()
    print("tones_fuzz: seed %d, %d case(s) identical to the model in %.1f s" % (a.seed, len(todo), time.time() - t0))


if __name__ == "__main__":
    main()
