"""The channelizer's integer spec (include/iqdemod.h: iqd_channelizer_*) stated once more, with one switchable defect.

channel(..., mutant=None) is the spec, written differently from chan_model.channel (a window matrix and one product per
rail instead of np.convolve; Python-integer phasor indices); tests/test_chan_corpus_host.py holds the two equal byte for
byte.  Every other value of `mutant` breaks exactly one step of the spec the way a kernel plausibly would.  A test input
has teeth for that step when the mutant's bytes differ from the model's: the corpus (tests/chan_corpus.py) and the
fuzzer's fixed slices (tools/chan_fuzz.py) are held to that before they go to the GPU."""
import numpy as np

MUTANTS = (
    "tap_round",      # g = (h P) >> 15: the + 2^14 dropped
    "tap_index",      # i_k = (k d mod 2^32) >> 19 (mod 4096) instead of >> 20
    "oldest_tap",     # the tap of x[n - (K - 1)] missing: a history one sample short
    "a_plus_1",       # A + 1 before (A + 128) >> 8: a wrong low bit of the lo tap plane
    "round_127",      # (A + 127) >> 8
    "shift_trunc",    # (A + 128) / 256 truncating toward zero instead of flooring
    "sat16_wrap",     # a wraps to int16 instead of saturating
    "phasor_late",    # the rotation phasor taken at n - 1
    "s_sign",         # ri = ai c + ar s
    "final_round",    # y = (r + 2^(21-L) - 1) >> (22-L)
    "sat8_127",       # the lower byte rail at -127
    "hi_plane",       # the hi tap plane one short of its range: g clipped to +-32512
)
TAP_MUTANTS = ("tap_round", "tap_index", "oldest_tap", "hi_plane")   # these change A itself; the others start from A
EXEMPT_FROM_FUZZ = ("final_round", "sat16_wrap")                     # the corpus owns them (rare under random inputs)


def taps(h, inc, P, mutant=None):
    """(gr, gi) as int64 arrays, tap by tap in Python integers."""
    gr, gi = [], []
    for k, hk in enumerate(int(v) for v in h):
        ph = (k * int(inc)) % (1 << 32)
        i = (ph >> 19) % 4096 if mutant == "tap_index" else ph >> 20
        rnd = 0 if mutant == "tap_round" else 1 << 14
        r, q = (hk * int(P[i][0]) + rnd) >> 15, (hk * int(P[i][1]) + rnd) >> 15
        if mutant == "hi_plane":
            r, q = max(-32512, min(32512, r)), max(-32512, min(32512, q))
        gr.append(r)
        gi.append(q)
    if mutant == "oldest_tap":
        gr[-1] = gi[-1] = 0
    return np.array(gr, np.int64), np.array(gi, np.int64)


def stage_A(wide_row, h, M, inc, P, m_range=None, mutant=None):
    """(Ar, Ai, n): the exact sums of outputs m_range (default: all of wide_row, a stream from sample 0), and their n."""
    u = np.asarray(wide_row, np.int64)
    K = len(h)
    n_out = len(u) // 2 // M
    m0, m1 = (0, n_out) if m_range is None else m_range
    n = np.arange(m0, m1, dtype=np.int64) * M + M - 1
    x = np.zeros((K - 1 + len(u) // 2, 2), np.int64)       # x[n < 0] = 0 in front
    x[K - 1:] = u.reshape(-1, 2) - 128
    gr, gi = taps(h, inc, P, mutant)
    # row j of the window matrix: x[n_j - (K - 1)] .. x[n_j], oldest first; the taps reversed to match
    first = int(n[0]) if len(n) else 0
    span = x[first:first + (len(n) - 1) * M + K] if len(n) else x[:0]
    win = np.lib.stride_tricks.sliding_window_view(span, K, axis=0)[::M] if len(n) else np.zeros((0, 2, K), np.int64)
    wr, wi = win[:, 0, :], win[:, 1, :]
    fr, fi = gr[::-1], gi[::-1]
    return wr @ fr - wi @ fi, wi @ fr + wr @ fi, n


def finish(Ar, Ai, n, inc, shift, P, mutant=None, stage_a=False):
    """From the exact sums to the output bytes (or, stage_a=True, to the int16 stage a)."""
    def to_a(A):
        if mutant == "a_plus_1":
            A = A + 1
        if mutant == "round_127":
            v = (A + 127) >> 8
        elif mutant == "shift_trunc":
            t = A + 128
            v = np.where(t < 0, -((-t) >> 8), t >> 8)
        else:
            v = (A + 128) >> 8
        if mutant == "sat16_wrap":
            return ((v + 32768) & 0xffff) - 32768
        return np.minimum(np.maximum(v, -32768), 32767)

    ar, ai = to_a(Ar), to_a(Ai)
    if stage_a:
        return ar, ai
    nn = n - 1 if mutant == "phasor_late" else n
    idx = np.array([((int(v) * int(inc)) % (1 << 32)) >> 20 for v in nn], np.int64)
    Pt = np.asarray(P, np.int64)
    c, s = Pt[idx, 0], Pt[idx, 1]
    rr = ar * c + ai * s
    ri = ai * c + ar * s if mutant == "s_sign" else ai * c - ar * s
    L = int(shift)
    rnd = (1 << (21 - L)) - (1 if mutant == "final_round" else 0)
    lo = -127 if mutant == "sat8_127" else -128
    out = np.empty(2 * len(n), np.uint8)
    for at, r in ((0, rr), (1, ri)):
        y = np.minimum(np.maximum((r + rnd) >> (22 - L), lo), 127)
        out[at::2] = (y + 128).astype(np.uint8)
    return out


def channel(wide_row, h, M, inc, shift, P, m_range=None, stage_a=False, mutant=None):
    """chan_model.channel's arguments and result; mutant=None is the spec, a name of MUTANTS the spec with that defect."""
    assert mutant is None or mutant in MUTANTS, mutant
    Ar, Ai, n = stage_A(wide_row, h, M, inc, P, m_range, mutant if mutant in TAP_MUTANTS else None)
    return finish(Ar, Ai, n, inc, shift, P, None if mutant in TAP_MUTANTS else mutant, stage_a)


def all_outputs(wide_row, h, M, inc, shift, P, m_range=None):
    """{None: the spec's bytes, mutant: its bytes} - the sums shared by the mutants that start from A."""
    Ar, Ai, n = stage_A(wide_row, h, M, inc, P, m_range)
    out = {None: finish(Ar, Ai, n, inc, shift, P)}
    for mu in MUTANTS:
        if mu in TAP_MUTANTS:
            out[mu] = finish(*stage_A(wide_row, h, M, inc, P, m_range, mu), inc, shift, P)
        else:
            out[mu] = finish(Ar, Ai, n, inc, shift, P, mu)
    return out
