"""Diagnostic: randomized packet-decoder runs on an MI355X, every array bit for bit against the model written from the header
(include/iqdemod_fsk.h; tests/fsk_model.py).

    python tools/fsk_fuzz.py [--seed S] [--cases N]        a campaign
    python tools/fsk_fuzz.py --seed S --case I             one case again

Case I of seed S is drawn from numpy's default_rng([S, I]) and from nothing else, so (seed, index) names a case on every
machine.  A case is drawn without a GPU (draw) and then run (run_case; gpu=False runs the model alone).  About every second
parameter comes from a list of edges, the rest at random, all inside the ranges the header documents.  Refusals are not fuzzed.

  modem     W around {2, 7, 8, 63, 64}, channels around a wave's 64; the tones of an 8-samples-per-bit modem, of Bell 202 at
            8 kS/s or at random; baud_inc over its whole range; loop_shift 1 .. 8; NRZI or not; the rectangular window, a
            random one, +-32512; min_len 3 .. 6, max_len up to 12 (so that frames overflow) or 1024
  samples   per channel: frames of the modem's own audio (random payloads, some too short, too long, with a bad FCS or aborted)
            under noise, noise alone, silence, +-32768
  calls     one to five, n from {0, 1, W - 1, W, 31, 32, 33, 64, 65, 255, 256, 257} or at random, row_stride >= n, rows 2-byte
            aligned only; counts (0 and above n among them) or none; bits or none; the host form or the device form; a reset
            in between"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                     # noqa: E402
from rtlsdrdiags_amd import fsk                        # noqa: E402
from tests import fsk_model as fm                      # noqa: E402
import pcm_fuzz_common as pf                           # noqa: E402
from pcm_fuzz_common import Buffers, case_rng, pick    # noqa: E402,F401 (Buffers: the tests' rig)

W_EDGES = (2, 7, 8, 63, 64)
C_EDGES = (1, 2, 63, 64, 65)
N_EDGES = (0, 1, 31, 32, 33, 64, 65, 255, 256, 257)
SLICE = (9402, 300)            # (seed, cases): tests/test_gpu_fsk_fuzz.py's
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def line_bits(rng, cfg):
    """flags and frames: most good, some too short, too long, with a bad FCS or cut by an abort"""
    bits = FLAG * int(rng.integers(2, 5))
    for _ in range(int(rng.integers(1, 4))):
        u = rng.random()
        size = int(rng.integers(1, 7)) if u < 0.7 else pick(rng, (cfg["min_len"] - 3, cfg["min_len"] - 2, cfg["max_len"] - 2, cfg["max_len"] - 1))
        size = min(max(size, 0), 40)
        payload = bytes(rng.integers(0, 256, size).astype(np.uint8)) if rng.random() < 0.8 else bytes([pick(rng, (0xff, 0x7e, 0x00))] * size)
        body = fm.hdlc_bits([payload], 0, 0, 0, bad_fcs=(0,) if rng.random() < 0.15 else ())
        if rng.random() < 0.1:
            body = body[:int(rng.integers(1, len(body)))] + [1] * int(rng.integers(7, 10)) + [0]
        bits += body + (FLAG if rng.random() < 0.5 else FLAG + [1, 1, 1, 1, 1, 1, 0] if rng.random() < 0.3 else FLAG * 2)
    return bits


def draw(seed, index, phasor):
    """dict(C, cfg and window for fm.Model / fsk.Fsk, steps: ("reset",) or ("run", pcm, n, count, want_bits, form))"""
    rng = case_rng(seed, index)
    W = pick(rng, W_EDGES) if rng.random() < 0.6 else int(rng.integers(2, 65))
    C = pick(rng, C_EDGES) if rng.random() < 0.4 else int(rng.integers(1, 40))
    u = rng.random()
    if u < 0.45:
        W = 8                                                         # a modem whose own audio decodes: frames, not only bits
    if u < 0.5:
        tones = dict(mark_inc=1 << 29, space_inc=1 << 30, baud_inc=1 << 29)
    elif u < 0.65:
        tones = {k: v for k, v in fm.afsk1200(8000).items() if k in ("mark_inc", "space_inc", "baud_inc")}
    else:
        tones = dict(mark_inc=int(rng.integers(0, 2 ** 32)), space_inc=int(rng.integers(0, 2 ** 32)),
                     baud_inc=pick(rng, (1 << 20, (1 << 31) - 1)) if rng.random() < 0.3 else int(2 ** rng.uniform(20, 31)))
    tones["baud_inc"] = min(max(tones["baud_inc"], 1 << 20), (1 << 31) - 1)
    min_len = int(rng.integers(3, 7))
    cfg = dict(tones, corr_len=W, loop_shift=int(rng.integers(1, 9)), flags=int(rng.random() < 0.7), min_len=min_len,
               max_len=1024 if rng.random() < 0.2 else int(rng.integers(min_len, 13)))
    u = rng.random()
    window = None if u < 0.4 else rng.integers(-32512, 32513, W).astype(np.int16) if u < 0.8 else np.full(W, pick(rng, (32512, -32512)), np.int16)
    own = W == 8 and tones["baud_inc"] >= 1 << 28                     # the modem's own audio is worth making
    stream = []
    for c in range(C):
        if own and rng.random() < 0.8:
            levels = line_bits(rng, cfg)
            levels = fm.nrzi_levels(levels) if cfg["flags"] else levels
            stream.append(np.concatenate([np.zeros(int(rng.integers(0, 9)), np.int64),
                                          fm.afsk(levels, phasor, cfg["mark_inc"], cfg["space_inc"], cfg["baud_inc"], int(2 ** rng.uniform(8, 14.9)))]))
        else:
            stream.append(np.zeros(0, np.int64))
    at = np.zeros(C, np.int64)
    steps = []
    for _ in range(int(rng.integers(1, 6))):
        if steps and rng.random() < 0.15:
            steps.append(("reset",))
        edges = N_EDGES + (W - 1, W)
        n = pick(rng, edges) if rng.random() < 0.5 else int(rng.integers(0, 900))
        stride = n + int(pick(rng, (0, 1, 3, 8)))
        pcm = rng.integers(-32768, 32768, (C, max(stride, 1))).astype(np.int16)       # (what lies behind n is never read)
        count = None
        if rng.random() < 0.4:
            count = rng.integers(0, n + 3, C).astype(np.uint32)
            count[int(rng.integers(C))] = pick(rng, (0, n, n + 7))
        for c in range(C):
            u = rng.random()
            amp = int(2 ** rng.uniform(2, 15))
            seg = rng.integers(-amp, amp + 1, n)
            if len(stream[c]) > at[c]:
                m = n if count is None else min(int(count[c]), n)
                part = stream[c][at[c]:at[c] + m]
                seg = seg // 8
                seg[:len(part)] += part
                at[c] += m
            elif u < 0.2:
                seg = np.zeros(n, np.int64)
            elif u < 0.3:
                seg = np.where(rng.integers(0, 2, n) == 0, 32767, -32768)
            elif u < 0.35:
                seg = np.full(n, -32768)
            pcm[c, :n] = np.clip(seg, -32768, 32767)
        steps.append(("run", pcm, n, count, rng.random() < 0.7, "host" if rng.random() < 0.3 else "device"))
    return dict(seed=seed, index=index, C=C, cfg=cfg, window=window, steps=steps)


def run_device(eng, bufs, t, pcm, n, count, want_bits):
    C, stride = pcm.shape
    F, Bw, Bc = t.max_frames(n), t.max_bit_words(n), t.max_bytes(n)
    p_pcm, p_cnt = pf.upload_rows(eng, bufs, pcm, count)
    p_nb, p_nf = bufs.get("nb", C * 4), bufs.get("nf", C * 4)
    p_bits, p_fr, p_by = bufs.get("bits", C * Bw * 4 + 16), bufs.get("frames", C * F * 24 + 16), bufs.get("bytes", C * Bc + 16)
    t.run_device(p_pcm, stride, n, p_nb, p_nf, p_fr, p_by, bits_dev=p_bits if want_bits else 0, count_dev=p_cnt)
    eng.synchronize()
    nb, nf = eng.dev_download(p_nb, C * 4, np.uint32), eng.dev_download(p_nf, C * 4, np.uint32)
    bits = np.zeros((C, Bw), np.uint32) if want_bits else None
    frames, data = np.zeros((C, F), fsk.FSK_FRAME), np.zeros((C, Bc), np.uint8)
    if n:
        if want_bits:
            bits = eng.dev_download(p_bits, C * Bw * 4, np.uint32).reshape(C, Bw)
        frames = eng.dev_download(p_fr, C * F * 24).view(fsk.FSK_FRAME).reshape(C, F)
        data = eng.dev_download(p_by, C * Bc, np.uint8).reshape(C, Bc)
    return nb, bits, nf, frames, data


def run_case(case, phasor, eng=None, bufs=None, gpu=True):
    """the model's results and every channel's state; with gpu, the library's held against them (AssertionError names the case
    and the step)"""
    m = fm.Model(case["C"], phasor, window=case["window"], **case["cfg"])
    out = pf.run_case(case, m, lambda: fsk.Fsk(eng, case["C"], window=case["window"], **case["cfg"]),
                      lambda t, *step: run_device(eng, bufs, t, *step), "want_bits",
                      [("n_bits", pf.equal), ("bits", None), ("n_frames", pf.equal), ("frames", pf.records), ("bytes", pf.equal)], gpu)
    return out, [m.state(c) for c in range(case["C"])]


if __name__ == "__main__":
    pf.main("fsk_fuzz", SLICE, draw, run_case)
