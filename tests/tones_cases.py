"""The inputs of tests/test_gpu_tones.py, proven against the defects of tones_model.py by tests/test_tones_host.py.

A case is one tone bank (channels, frame length, tones, window, thresholds) and a list of steps: ("run", pcm [C, stride] int16,
n, count or None) and ("reset",).  Shapes are the smallest at which a kernel can still go wrong: L in {32, 64, 96, 4096, 8192},
T in {1, 2, 15, 16, 17, 50, 64} (2 T straddles the MFMA tile's 16 rows), C in {1, 15, 16, 17, 65} (the workgroup's 16 channels),
n in {0, 1, L - 1, L, L + 1, 3 L + 5} in sequences so that frames straddle one, two and three calls, row_stride > n, counts that
differ (0 and > n among them).  Every signal is made of integers (the library's phasor table and a seeded generator), so the
inputs are the same on every machine.  `blind`: the defects of tones_model.DEFECTS that leave this case's result unchanged;
test_tones_host.py holds the set against the model, and every defect is seen by some case."""
import numpy as np

from tests import tones_model as tm

CTCSS_MHZ = [67000, 69300, 71900, 74400, 77000, 79700, 82500, 85400, 88500, 91500, 94800, 97400, 100000, 103500, 107200, 110900,
             114800, 118800, 123000, 127300, 131800, 136500, 141300, 146200, 151400, 156700, 159800, 162200, 165500, 167900,
             171300, 173800, 177300, 179900, 183500, 186200, 189900, 192800, 196600, 199500, 203500, 206500, 210700, 218100,
             225700, 229100, 233600, 241800, 250300, 254100]
PCM_RATE = 8000


# case -> the defects it is blind to (a case sees every other one); why, by group: a case without a tie does not see the tie
# rules, one whose products stay below 2^64 not the wrapped ratio, one with whole rows not the counts, one whose channels all
# complete the same frames not the tail, one without reset not reset, one with open = 1 / hold = 0 or without a tone in force
# not the decision's edges, one of a single call not the carry.  tests/test_tones_host.py holds each set against the model.
BLIND = {
    "l32_t17_c17_cuts":
        "count_ignored ratio_wrap64 reset_keeps_frame tie_high",
    "l64_t15_c15_counts":
        "miss_ge_hold ratio_wrap64 reset_keeps_frame switch_loses_open tie_high",
    "l96_t16_c16":
        "count_ignored ratio_wrap64 reset_keeps_frame tie_high",
    "l4096_ctcss_c65":
        "count_ignored miss_ge_hold ratio_wrap64 reset_keeps_frame switch_loses_open tail_not_zeroed tie_high",
    "l8192_bound_t64":
        "count_ignored low_plane_unsigned miss_ge_hold reset_keeps_frame switch_loses_open",
    "alternating_t1":
        "count_ignored miss_ge_hold phase_from_call ratio_wrap64 reset_keeps_frame second_is_best switch_loses_open tail_not_zeroed tie_high",
    "alternating_t2":
        "carry_dropped count_ignored phase_from_call ratio_wrap64 reset_keeps_frame switch_loses_open tail_not_zeroed tie_high trunc_shift",
    "tie_of_two":
        "carry_dropped count_ignored phase_from_call ratio_wrap64 reset_keeps_frame switch_loses_open tail_not_zeroed trunc_shift",
    "tie_refused_by_ratio":
        "carry_dropped count_ignored miss_ge_hold phase_from_call ratio_wrap64 reset_keeps_frame switch_loses_open tail_not_zeroed trunc_shift",
    "silence_hits":
        "carry_dropped count_ignored low_plane_unsigned no_round phase_from_call ratio_wrap64 reset_keeps_frame switch_loses_open trunc_shift",
    "silence_misses":
        "carry_dropped count_ignored low_plane_unsigned miss_ge_hold no_round phase_from_call ratio_wrap64 reset_keeps_frame switch_loses_open trunc_shift",
    "decision_open2_hold1":
        "carry_dropped count_ignored phase_from_call ratio_wrap64 reset_keeps_frame tail_not_zeroed trunc_shift",
    "decision_switch_in_one_frame":
        "count_ignored ratio_wrap64 reset_keeps_frame trunc_shift",
    "decision_open3_hold2":
        "carry_dropped count_ignored phase_from_call ratio_wrap64 reset_keeps_frame switch_loses_open tail_not_zeroed trunc_shift",
    "reset_in_mid_frame":
        "carry_dropped count_ignored miss_ge_hold phase_from_call ratio_wrap64 switch_loses_open tie_high",
}


class Case:
    def __init__(self, name, C, L, incs, steps, window=None, **thresholds):
        self.name, self.C, self.L, self.incs, self.steps, self.window = name, C, L, [int(d) for d in incs], steps, window
        self.thresholds = dict(dict(min_power=0, ratio_q8=256, energy_q8=0, open=1, hold=0), **thresholds)
        self.blind = frozenset(BLIND[name].split())

    def model(self, phasor, defect=None):
        return tm.Model(self.C, self.L, self.incs, phasor, window=self.window, defect=defect, **self.thresholds)


def tone(phasor, inc, amp, n, start=0):
    """amp cos(2 pi inc (start + k) / 2^32), k < n, from the table's cosines: integers only"""
    k = (np.arange(n, dtype=np.uint64) + np.uint64(start)) * np.uint64(int(inc))
    i = ((k & np.uint64(0xffffffff)) >> np.uint64(20)).astype(np.int64)
    return (int(amp) * phasor[i, 0].astype(np.int64)) >> 15


def noise(rng, shape, amp):
    return rng.integers(-amp, amp + 1, shape).astype(np.int64)


def steps_of(x, cuts, pad=3, counts=None):
    """x [C, N] cut into calls at `cuts` (lengths); each call's rows are padded by `pad` samples of another value, so
    row_stride > n; counts: per call None or [C]"""
    out, at = [], 0
    for i, n in enumerate(cuts):
        rows = np.full((x.shape[0], n + pad), -12345, np.int16)
        rows[:, :n] = x[:, at:at + n]
        out.append(("run", rows, n, None if counts is None else counts[i]))
        at += n
    assert at <= x.shape[1]
    return out


def bin_inc(L, k):
    return (k << 32) // L


def run_model(case, phasor, defect=None):
    """every step's result: a list of (n_frames, frames, power) and the final states"""
    m = case.model(phasor, defect)
    out = []
    for s in case.steps:
        if s[0] == "reset":
            m.reset()
        else:
            out.append(m.run(s[1], s[2], s[3]))
    return out, [m.state(c) for c in range(case.C)]


def same(a, b):
    (ra, sa), (rb, sb) = a, b
    return sa == sb and len(ra) == len(rb) and all(np.array_equal(x, y) for u, v in zip(ra, rb) for x, y in zip(u, v))


def build(phasor):
    rng = np.random.default_rng(20240611)
    cases = []

    # noise and a tone per channel, every cut length of L = 32; 2 T = 34 rows: three tiles, the last with two rows
    L, C, T = 32, 17, 17
    incs = [bin_inc(L, 1 + t % 15) + 12345 * t for t in range(T)]
    N = 0 + 1 + 31 + 32 + 33 + 101 + 5
    x = noise(rng, (C, N), 3000) + np.stack([tone(phasor, incs[c % T], 9000, N) for c in range(C)])
    cases.append(Case("l32_t17_c17_cuts", C, L, incs, steps_of(x, [0, 1, 31, 32, 33, 101, 5])))

    # counts that differ, 0 and > n among them; 15 channels and 15 tones
    L, C, T = 64, 15, 15
    incs = [bin_inc(L, 2 + t) for t in range(T)]
    cuts = [65, 197, 63, 1, 0, 64]
    x = noise(rng, (C, sum(cuts)), 20000)
    counts = [rng.integers(0, n + 3, C).astype(np.uint32) for n in cuts]
    counts[1][0], counts[1][1], counts[1][2] = 0, 197 + 7, 64
    cases.append(Case("l64_t15_c15_counts", C, L, incs, steps_of(x, cuts, pad=1, counts=counts), open=2, hold=1, ratio_q8=300))

    # L = 96: no power of two, one and a half K-chunks; 16 channels, 16 tones: whole tiles
    L, C, T = 96, 16, 16
    incs = [int(v) for v in rng.integers(0, 2 ** 32, T)]
    cuts = [95, 1, 96, 97, 293]
    x = noise(rng, (C, sum(cuts)), 32767)
    cases.append(Case("l96_t16_c16", C, L, incs, steps_of(x, cuts), energy_q8=3, min_power=1000))

    # the workload's shape in small: 50 CTCSS tones, L = 4096, default window and thresholds; 65 channels (five workgroups,
    # the last with one channel), a tone of amplitude 1000 under noise in each
    L, C = 4096, 65
    incs = [tm.phase_inc(f, PCM_RATE) for f in CTCSS_MHZ]
    cuts = [4095, 4097, 5]
    x = noise(rng, (C, sum(cuts)), 200) + np.stack([tone(phasor, incs[(7 * c) % 50], 1000, sum(cuts)) for c in range(C)])
    cases.append(Case("l4096_ctcss_c65", C, L, incs, steps_of(x, cuts), ratio_q8=512, open=2, hold=1))

    # the accumulator bound: L = 8192, w = 32767, every sample -32768, 64 tones of which 0 and 1 are DC (|A| = 2^43 and a tie)
    # and 2 is the Nyquist tone; ratio_q8 = 64775 on p_best = p_second = 2^54: the product passes 2^64
    L, C, T = 8192, 1, 64
    incs = [0, 0, 2 ** 31] + [int(v) for v in rng.integers(0, 2 ** 32, T - 3)]
    x = np.full((C, 8192 + 8191 + 1 + 3 * 8192 + 5), -32768, np.int64)
    cases.append(Case("l8192_bound_t64", C, L, incs, steps_of(x, [8192, 8191, 1, 3 * 8192 + 5]), window=np.full(L, 32767, np.int16),
                      ratio_q8=64775))

    # alternating +-32767: all of it in the Nyquist tone, which sits exactly on a table step; one tone only (second = NONE)
    L = 64
    x = np.tile(np.array([32767, -32767], np.int64), 100)[None, :]
    cases.append(Case("alternating_t1", 1, L, [2 ** 31], steps_of(x, [63, 65, 64]), window=np.full(L, -32767, np.int16), energy_q8=1 << 20))
    cases.append(Case("alternating_t2", 1, L, [2 ** 30, 2 ** 31], steps_of(x, [64, 64, 64]), min_power=1))

    # two equal increments: a tie for best; the third tone far behind
    L = 32
    incs = [bin_inc(L, 9), bin_inc(L, 4), bin_inc(L, 4)]
    x = tone(phasor, incs[1], 12000, 3 * L)[None, :]
    cases.append(Case("tie_of_two", 1, L, incs, steps_of(x, [L, 2 * L]), ratio_q8=256))
    cases.append(Case("tie_refused_by_ratio", 1, L, incs, steps_of(x, [L, 2 * L]), ratio_q8=257))

    # silence: E = 0 and every p = 0, best = 0; a hit with every threshold 0, none with min_power = 1
    x = np.zeros((2, 3 * 32 + 5), np.int64)
    cases.append(Case("silence_hits", 2, 32, incs, steps_of(x, [3 * 32 + 5]), energy_q8=1 << 20, ratio_q8=65535))
    cases.append(Case("silence_misses", 2, 32, incs, steps_of(x, [3 * 32 + 5]), min_power=1))

    # the decision recurrence, frame by frame: A = tone 0, B = tone 1, - = silence (no hit: min_power)
    L = 32
    incs = [bin_inc(L, 4), bin_inc(L, 9)]
    unit = {"A": tone(phasor, incs[0], 8000, L), "B": tone(phasor, incs[1], 8000, L), "-": np.zeros(L, np.int64)}

    def script(text):
        return np.concatenate([unit[ch] for ch in text])[None, :]

    text = "A-AA-A--AABBA-BB-B--"
    cases.append(Case("decision_open2_hold1", 1, L, incs, steps_of(script(text), [L * 7, L * 13]), min_power=1000, open=2, hold=1))
    text = "AABBA-BAB--A"
    cases.append(Case("decision_switch_in_one_frame", 1, L, incs, steps_of(script(text), [L * 3 + 5, L * 9 - 5]), min_power=1000, open=1, hold=0))
    text = "AAA-B-AB--B---BBB"
    cases.append(Case("decision_open3_hold2", 1, L, incs, steps_of(script(text), [L * 17]), min_power=1000, open=3, hold=2))

    # reset in the middle of a frame: the next frame starts with the next call's first sample
    L, C = 64, 3
    incs = [bin_inc(L, 3), bin_inc(L, 11)]
    x = noise(rng, (C, 37 + 64 + 100), 15000)
    st = steps_of(x, [37, 64, 100])
    cases.append(Case("reset_in_mid_frame", C, L, incs, [st[0], ("reset",), st[1], st[2]], open=1, hold=3))
    return cases


# ---- the chain test's signal (tests/test_gpu_tones_chain.py; its CPU half is in tests/test_tones_host.py) ----
CHAIN_TONE = 12                 # CTCSS_MHZ[12]: 100.0 Hz
CHAIN_FRAMES = 3                # frames of 4096 PCM samples: 32 IQ samples each
CHAIN_DEVIATION = (600.0, 2500.0)   # Hz: of the sub-audible tone and of the 1 kHz audio tone above it


def chain_iq(n_frames=CHAIN_FRAMES, seed=7):
    """An FM carrier at -Fs/4 carrying CTCSS_MHZ[CHAIN_TONE] under a 1 kHz tone, as offset-binary uint8 I/Q at 256 kS/s:
    n_frames x 4096 x 32 samples.  The sub-audible deviation is a land-mobile one (some 15 % of the channel's)."""
    from rtlsdrdiags_amd import synth
    rng = np.random.default_rng(seed)
    n = np.arange(n_frames * 4096 * 32, dtype=np.float64)
    f_sub = CTCSS_MHZ[CHAIN_TONE] / 1000.0
    phase = (-0.5 * np.pi * n + (CHAIN_DEVIATION[0] / f_sub) * np.sin(2 * np.pi * f_sub * n / synth.FS)
             + (CHAIN_DEVIATION[1] / 1000.0) * np.sin(2 * np.pi * 1000.0 * n / synth.FS))
    return synth._finish(60.0 * np.exp(1j * phase), 3.0, rng)
