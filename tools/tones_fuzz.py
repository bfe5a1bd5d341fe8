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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                     # noqa: E402
from rtlsdrdiags_amd import tones                      # noqa: E402
from tests import tones_model as tm                    # noqa: E402
import pcm_fuzz_common as pf                           # noqa: E402
from pcm_fuzz_common import Buffers, case_rng, pick    # noqa: E402,F401 (Buffers: the tests' rig)

L_EDGES = (32, 64, 96, 128, 160, 256)
T_EDGES = (1, 2, 7, 8, 9, 15, 16, 17, 33, 64)
C_EDGES = (1, 2, 15, 16, 17, 33)
SLICE = (9401, 300)            # (seed, cases): tests/test_gpu_tones_fuzz.py's


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


def run_device(eng, bufs, t, pcm, n, count, want_power):
    C, stride = pcm.shape
    F, T = t.max_frames(n), t.n_tones
    p_pcm, p_cnt = pf.upload_rows(eng, bufs, pcm, count)
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
    m = tm.Model(case["C"], case["L"], case["incs"], phasor, window=case["window"], **case["cfg"])
    return pf.run_case(case, m, lambda: tones.Tones(eng, case["C"], np.array(case["incs"], np.uint32), frame_len=case["L"],
                                                    window=case["window"], **case["cfg"]),
                       lambda t, *step: run_device(eng, bufs, t, *step), "want_power",
                       [("n_frames", pf.equal), ("frames", pf.records), ("power", None)], gpu)


if __name__ == "__main__":
    pf.main("tones_fuzz", SLICE, draw, run_case)
