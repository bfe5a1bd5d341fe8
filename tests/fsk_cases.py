"""The inputs of tests/test_gpu_fsk.py, proven against the defects of fsk_model.py by tests/test_fsk_host.py.

A case is one decoder (channels, correlators, clock, framing) and a list of steps: ("run", pcm [C, stride] int16, n, count or
None) and ("reset",).  Shapes are the smallest at which a kernel can still go wrong: W in {2, 7, 8, 63, 64}, 1, 2, 63, 64 and 65
channels (a wave's 64 lanes, the walk's one wave per channel), n in {0, 1, W - 1, W, 31, 32, 33, 64, 65} and a few hundred (the
decision words of 32, a wave's ballot of 64, the tile of 256), row_stride > n, counts that differ.  Every signal is made of
integers (the library's phasor table and a seeded generator), so the inputs are the same on every machine.  Most framing cases
use the `T8` modem: 8 samples per bit, one cycle of the mark tone and two of the space tone per bit over a window of one bit -
the two tones are orthogonal over the window, so the decisions are the transmitted levels half a bit late.
`BLIND`: the defects of fsk_model.DEFECTS that leave a case's result unchanged; test_fsk_host.py holds the sets against the
model, and every defect is seen by some case."""
import numpy as np

from tests import fsk_model as fm

T8 = dict(corr_len=8, mark_inc=1 << 29, space_inc=1 << 30, baud_inc=1 << 29, loop_shift=3, flags=fm.NRZI, min_len=3, max_len=8)
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]

# case -> the defects it is blind to (a case sees every other one).  tests/test_fsk_host.py holds each set against the model.
BLIND = {
    "t8_every_bit_a_call":
        "count_ignored max_len_off",
    "t8_shared_flags":
        "count_ignored history_dropped max_len_off phase_from_stream",
    "t8_lengths_bad_fcs_abort":
        "count_ignored history_dropped phase_from_stream",
    "w7_c63_nrzi_off_small_n":
        "count_ignored max_len_off nrzi_polarity phase_from_stream",
    "t8_c64_counts":
        "max_len_off soft_ge",
    "w64_bound_soft_zero":
        "count_ignored crc_init_0 end_sample_off fcs_swapped lb_minus_8 max_len_off msb_first nbits_kept nrzi_polarity phase_from_stream",
    "w2_c65_fastest_clock":
        "count_ignored crc_init_0 end_sample_off fcs_swapped lb_minus_8 msb_first soft_ge",
    "w63_slowest_clock":
        "count_ignored crc_init_0 end_sample_off fcs_swapped lb_minus_8 max_len_off msb_first nbits_kept nudge_after_inc soft_ge stuff_after_six",
    "afsk1200_noise":
        "coef_no_round count_ignored max_len_off phase_from_stream soft_ge",
}


class Case:
    def __init__(self, name, C, cfg, steps, window=None):
        self.name, self.C, self.cfg, self.steps, self.window = name, C, dict(cfg), steps, window
        self.blind = frozenset(BLIND.get(name, "").split())

    def model(self, phasor, defect=None):
        return fm.Model(self.C, phasor, window=self.window, defect=defect, **self.cfg)


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
    assert at <= x.shape[1], (at, x.shape)
    return out


def audio(phasor, cfg, bits, amp=8000, tail=24):
    """the line bits through NRZI (where the modem has it) as audio, with `tail` samples of silence behind"""
    levels = fm.nrzi_levels(bits) if cfg["flags"] & fm.NRZI else list(bits)
    x = fm.afsk(levels, phasor, cfg["mark_inc"], cfg["space_inc"], cfg["baud_inc"], amp)
    return np.concatenate([x, np.zeros(tail, np.int64)])


def stuffed(payload, bad=False):
    """a payload's bits with its FCS, stuffed, without flags"""
    return fm.hdlc_bits([payload], 0, 0, 0, bad_fcs=(0,) if bad else ())


def run_model(case, phasor, defect=None):
    """every step's result: a list of (n_bits, bits, n_frames, frames, bytes) and the final states"""
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


def frames_found(result):
    """[(channel, end_sample, payload)] over all of a case's calls"""
    return [(c, int(r["end_sample"]), bytes(data[c, r["offset"]:r["offset"] + r["len"]]))
            for _, _, nf, frames, data in result[0] for c in range(len(nf)) for r in frames[c, :nf[c]]]


def build(phasor):
    rng = np.random.default_rng(20240712)
    cases = []

    def pad_rows(rows):
        n = max(len(r) for r in rows)
        return np.stack([np.concatenate([r, np.zeros(n - len(r), np.int64)]) for r in rows])

    # one short frame with stuffed zeros (0xff, 0x3e: five ones across a byte boundary), every call 8 samples: a cut at every
    # bit of both flags, inside the stuffed zeros and mid-byte; the second channel three samples late, its cuts inside the bits
    bits = FLAG * 3 + stuffed(b"\xff\x3e\xa7") + FLAG * 2
    x = audio(phasor, T8, bits)
    x = pad_rows([x, np.concatenate([np.zeros(3, np.int64), x])])
    cases.append(Case("t8_every_bit_a_call", 2, T8, steps_of(x, [8] * (x.shape[1] // 8))))

    # two frames that share one flag, then two flags that share their zero and a third frame; cut so that the first frame
    # spans three calls and the second and third close in one; channel 1 carries other payloads
    def shared(p):
        return FLAG * 3 + stuffed(p[0]) + FLAG + stuffed(p[1]) + FLAG + [1, 1, 1, 1, 1, 1, 0] + stuffed(p[2]) + FLAG * 2

    x = pad_rows([audio(phasor, T8, shared([b"\x01\x02\x03\x04", b"\xf0", b"\x7e\x7e"])),
                  audio(phasor, T8, shared([b"\xaa", b"\x55\x00\xff", b"\x1f\xf8\x00"]))])
    N = x.shape[1]
    cases.append(Case("t8_shared_flags", 2, T8, steps_of(x, [250, 250, 200, N - 700])))

    # the length limits, min_len = 5 and max_len = 8 with the FCS: payloads of 2 (too short: dropped), 3 (min_len), 6 (max_len)
    # and 7 bytes (overflows: dropped); then a bad FCS, an abort of eight ones inside a frame, and a good frame behind it
    cfg = dict(T8, min_len=5)
    bits = (FLAG * 3 + stuffed(b"\x11\x22") + FLAG + stuffed(b"\x33\x44\x55") + FLAG + stuffed(b"\x01\x02\x03\x04\x05\x06") + FLAG +
            stuffed(b"\x01\x02\x03\x04\x05\x06\x07") + FLAG + stuffed(b"\x0a\x0b\x0c\x0d", bad=True) + FLAG +
            stuffed(b"\x21\x43")[:20] + [1] * 8 + [0] + FLAG * 2 + stuffed(b"\x99\x88\x77\x66") + FLAG * 2)
    x = audio(phasor, cfg, bits)[None, :]
    cases.append(Case("t8_lengths_bad_fcs_abort", 1, cfg, steps_of(x, [x.shape[1]])))

    # NRZI off, loop_shift 1, W = 7 on 63 channels with every small n; noise of a quarter of the amplitude on top;
    # a reset in the middle of the stream, then the frame again
    cfg = dict(T8, corr_len=7, flags=0, loop_shift=1)
    C = 63
    bits = FLAG * 4 + stuffed(b"\xde\xad\xbe\xef") + FLAG * 2
    rows = [np.concatenate([np.zeros(c % 5, np.int64), audio(phasor, cfg, bits)]) for c in range(C)]
    x = pad_rows(rows)
    x = np.concatenate([x, x], axis=1)
    x = x + noise(rng, x.shape, 2000)
    half = x.shape[1] // 2
    cuts = [0, 1, 6, 7, 31, 32, 33, 64, 65]
    st = steps_of(x, cuts + [half - sum(cuts) - 100, 100] + [half])
    cases.append(Case("w7_c63_nrzi_off_small_n", C, cfg, st[:-1] + [("reset",)] + st[-1:]))

    # counts: rows of 0, of partial length and beyond n; 64 channels; loop_shift 8
    cfg = dict(T8, loop_shift=8)
    C = 64
    bits = FLAG * 4 + stuffed(b"\x42\x24\x18") + FLAG * 3
    x = pad_rows([audio(phasor, cfg, bits) for c in range(C)]) + noise(rng, (C, len(audio(phasor, cfg, bits))), 500)
    N = x.shape[1]
    cuts = [N // 3, N // 3, N - 2 * (N // 3)]
    counts = [rng.integers(0, n + 3, C).astype(np.uint32) for n in cuts]
    counts[0][:4] = [0, cuts[0], cuts[0] + 9, 1]
    counts[1][:4] = [cuts[1], cuts[1], 0, cuts[1]]
    counts[2][:4] = [cuts[2], cuts[2], cuts[2], cuts[2]]
    cases.append(Case("t8_c64_counts", C, cfg, steps_of(x, cuts, pad=1, counts=counts)))

    # the accumulator bound: W = 64, the window at its limit, the mark tone DC and the space tone Nyquist; rows of -32768, of
    # +-32768 alternating, of zeros (soft == 0) and of +32767: |sum| = 64 x 127 x 32768, soft near +-2^57
    cfg = dict(corr_len=64, mark_inc=0, space_inc=1 << 31, baud_inc=1 << 28, loop_shift=2, flags=0, min_len=3, max_len=3)
    seg = 80
    alt = np.tile(np.array([-32768, 32767], np.int64), seg // 2)
    alt2 = np.tile(np.array([32767, -32768], np.int64), seg // 2)
    row0 = np.concatenate([np.full(seg, -32768, np.int64), alt, np.zeros(seg, np.int64), np.full(seg, 32767, np.int64), alt2, alt])
    x = np.stack([row0, np.roll(row0, 37), -1 - row0])
    cases.append(Case("w64_bound_soft_zero", 3, cfg, steps_of(x, [63, 64, 65, x.shape[1] - 192]), window=np.full(64, -32512, np.int16)))

    # W = 2 and W = 63 on full-scale noise, 65 channels and 1; baud_inc at both ends: a bit every 4096 samples and one every
    # two and a bit
    cfg = dict(corr_len=2, mark_inc=123456789, space_inc=3000000000, baud_inc=(1 << 31) - 1, loop_shift=1, flags=fm.NRZI, min_len=3, max_len=4)
    x = noise(rng, (65, 1 + 2 + 330), 32767)
    cases.append(Case("w2_c65_fastest_clock", 65, cfg, steps_of(x, [1, 2, 330])))
    cfg = dict(corr_len=63, mark_inc=phase(700, 8000), space_inc=phase(1900, 8000), baud_inc=1 << 20, loop_shift=1, flags=fm.NRZI, min_len=3,
               max_len=1024)
    x = noise(rng, (1, 62 + 63 + 9000), 32767)
    w = (np.arange(63) * 1000 - 31000).astype(np.int16)
    cases.append(Case("w63_slowest_clock", 1, cfg, steps_of(x, [62, 63, 9000]), window=w))

    # Bell 202 at 8 kS/s as set=afsk1200 has it: a 20-byte frame of min_len 17 + ... under noise, on two channels
    cfg = fm.afsk1200(8000)
    payload = bytes(rng.integers(0, 256, 20).astype(np.uint8))
    bits = [0, 0, 0] + FLAG * 4 + stuffed(payload) + FLAG * 2
    a = audio(phasor, cfg, bits)
    x = pad_rows([a, np.concatenate([np.zeros(11, np.int64), a])])
    x = x + noise(rng, x.shape, 1500)
    N = x.shape[1]
    cases.append(Case("afsk1200_noise", 2, cfg, steps_of(x, [257, 255, N - 512])))
    return cases


def phase(hz, rate):
    return fm.phase_inc(hz * 1000, rate)


# ---- the chain test's signal (tests/test_gpu_fsk_chain.py; its CPU half is in tests/test_fsk_host.py) ----
CHAIN_DEVIATION = 3000.0
CHAIN_SEED = 7


def chain_payload(seed=CHAIN_SEED):
    return bytes(np.random.default_rng(1000 + seed).integers(0, 256, 40).astype(np.uint8))


def chain_iq(seed=CHAIN_SEED, deviation=CHAIN_DEVIATION):
    """An FM carrier at -Fs/4, frequency-modulated by unit-amplitude continuous-phase 1200 / 2200 Hz audio, as offset-binary
    uint8 I/Q at 256 kS/s: 300 x 32 unmodulated samples, then three 0 bits, four flags, the 40-byte payload with its FCS and
    two flags in NRZI (a 0 bit is a change, the starting level is 1200 Hz), padded to whole 32768-sample blocks."""
    from rtlsdrdiags_amd import synth
    rng = np.random.default_rng(seed)
    bits = [0, 0, 0] + fm.hdlc_bits([chain_payload(seed)], 4, 1, 2)
    levels = fm.nrzi_levels(bits, level=0)            # a 0 bit first: the level before it is 2200 Hz, the first on 1200 Hz
    assert levels[0] == 1
    per_bit = synth.FS / 1200.0
    n_mod = int(np.ceil(len(levels) * per_bit))
    t = np.arange(n_mod)
    tone = np.where(np.array(levels)[np.minimum((t / per_bit).astype(np.int64), len(levels) - 1)] == 1, 1200.0, 2200.0)
    audio_phase = 2 * np.pi * np.cumsum(tone) / synth.FS
    m = np.concatenate([np.zeros(300 * 32), np.sin(audio_phase)])
    total = -(-len(m) // 32768) * 32768
    m = np.concatenate([m, np.zeros(total - len(m))])
    phase = -0.5 * np.pi * np.arange(total) + 2 * np.pi * deviation * np.cumsum(m) / synth.FS
    return synth._finish(60.0 * np.exp(1j * phase), 3.0, rng)
