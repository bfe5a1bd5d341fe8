"""GPU tier of the PCM packet decoder (include/iqdemod_fsk.h): every case of tests/fsk_cases.py bit for bit against
tests/fsk_model.py - the counts, the bit words, every record, the payload bytes, the zero tails, get_state - through run_device
on rows that are only 2-byte aligned and on output arrays filled with another value beforehand; then run against run_device,
bits_dev = NULL, two objects on one engine, one call against the same samples in two, and the launch count."""
import numpy as np
import pytest

from rtlsdrdiags_amd import capi, fsk
from tests import fsk_cases as fc
from tests import fsk_model as fm

pytestmark = pytest.mark.gpu

CLEARED = dict(samples=0, ph=0, prev=0, last=0, ones=0, in_frame=0, nbits=0, bad_fcs=0, frames_total=0)
LAUNCHES = 2            # the header's number for n > 0; one for n = 0


@pytest.fixture(scope="module")
def phasor():
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def cases(phasor):
    return {c.name: c for c in fc.build(phasor)}


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(n_channels=1)
    yield e
    e.close()


def make(eng, case, **over):
    return fsk.Fsk(eng, case.C, window=case.window, **dict(case.cfg, **over))


class DeviceCall:
    """one run_device call's arrays on the device: the rows from 2 bytes behind an aligned address on, the outputs filled with
    0xAB bytes"""

    def __init__(self, eng, t, pcm, n, count, want_bits=True):
        self.eng, self.t = eng, t
        C, stride = pcm.shape
        self.C, self.F, self.Bw, self.Bc = C, t.max_frames(n), t.max_bit_words(n), t.max_bytes(n)
        self.ptrs = []
        self.pcm = self._put(np.concatenate([np.zeros(1, np.int16), pcm.reshape(-1)])) + 2
        self.count = self._put(np.ascontiguousarray(count, np.uint32)) if count is not None else 0
        self.nb = self._put(np.full(C * 4, 0xAB, np.uint8))
        self.nf = self._put(np.full(C * 4, 0xAB, np.uint8))
        self.bits = self._put(np.full(max(C * self.Bw * 4, 16), 0xAB, np.uint8)) if want_bits else 0
        self.frames = self._put(np.full(max(C * self.F * 24, 16), 0xAB, np.uint8))
        self.bytes = self._put(np.full(max(C * self.Bc, 16), 0xAB, np.uint8))
        self.stride, self.n = stride, n

    def _put(self, a):
        p = self.eng.dev_alloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        self.eng.dev_upload(p, a)
        return p

    def run(self):
        self.t.run_device(self.pcm, self.stride, self.n, self.nb, self.nf, self.frames, self.bytes, bits_dev=self.bits, count_dev=self.count)

    def result(self):
        """(n_bits, bits or None, n_frames, frames, bytes); synchronises, frees"""
        self.eng.synchronize()
        C = self.C
        nb, nf = self.eng.dev_download(self.nb, C * 4, np.uint32), self.eng.dev_download(self.nf, C * 4, np.uint32)
        bits = np.zeros((C, self.Bw), np.uint32) if self.bits else None
        frames, data = np.zeros((C, self.F), fsk.FSK_FRAME), np.zeros((C, self.Bc), np.uint8)
        if self.n:
            if self.bits:
                bits = self.eng.dev_download(self.bits, C * self.Bw * 4, np.uint32).reshape(C, self.Bw)
            frames = self.eng.dev_download(self.frames, C * self.F * 24, np.uint8).view(fsk.FSK_FRAME).reshape(C, self.F)
            data = self.eng.dev_download(self.bytes, C * self.Bc, np.uint8).reshape(C, self.Bc)
        for p in self.ptrs:
            self.eng.dev_free(p)
        return nb, bits, nf, frames, data


def run_device(eng, t, pcm, n, count=None, want_bits=True):
    call = DeviceCall(eng, t, pcm, n, count, want_bits)
    call.run()
    return call.result()


def check(got, want, what):
    nb, bits, nf, frames, data = got
    assert np.array_equal(nb, want[0]), (what, "n_bits", nb, want[0])
    if bits is not None:
        assert bits.shape == want[1].shape and np.array_equal(bits, want[1]), (what, "bits")
    assert np.array_equal(nf, want[2]), (what, "n_frames", nf, want[2])
    for k in fm.FRAME.names:
        assert np.array_equal(frames[k], want[3][k]), (what, k, frames[k], want[3][k])
    assert frames.tobytes() == want[3].tobytes(), what
    assert data.shape == want[4].shape and np.array_equal(data, want[4]), (what, "bytes")


@pytest.mark.parametrize("name", list(fc.BLIND))
def test_corpus_case_bit_for_bit(eng, cases, phasor, name):
    case = cases[name]
    m, t = case.model(phasor), make(eng, case)
    try:
        assert t.state(case.C - 1) == CLEARED
        for n in (0, 1, 100, 2048):
            assert (t.max_frames(n), t.max_bit_words(n), t.max_bytes(n)) == (m.max_frames(n), m.max_bit_words(n), m.max_bytes(n)), n
        for i, s in enumerate(case.steps):
            if s[0] == "reset":
                m.reset()
                t.reset()
                continue
            check(run_device(eng, t, s[1], s[2], s[3]), m.run(s[1], s[2], s[3]), (name, i))
            assert t.state(0) == m.state(0), (name, i)
        for c in range(case.C):
            assert t.state(c) == m.state(c), (name, c)
    finally:
        t.close()


@pytest.mark.parametrize("name", ["t8_c64_counts", "t8_shared_flags", "w64_bound_soft_zero"])
def test_run_is_run_device(eng, cases, phasor, name):
    case = cases[name]
    m, t = case.model(phasor), make(eng, case)
    try:
        for i, s in enumerate(case.steps):
            check(t.run(s[1], s[2], s[3]), m.run(s[1], s[2], s[3]), (name, i))
        assert [t.state(c) for c in range(case.C)] == [m.state(c) for c in range(case.C)]
    finally:
        t.close()


def test_without_bits_the_rest_is_the_same(eng, cases, phasor):
    case = cases["t8_lengths_bad_fcs_abort"]
    m, t = case.model(phasor), make(eng, case)
    try:
        for i, s in enumerate(case.steps):
            got = run_device(eng, t, s[1], s[2], s[3], want_bits=False)
            assert got[1] is None
            check(got, m.run(s[1], s[2], s[3]), i)
        s = case.steps[-1]
        host = t.run(s[1], s[2], s[3], want_bits=False)
        assert host[1] is None
        check(host, m.run(s[1], s[2], s[3]), "host")
    finally:
        t.close()


def test_two_objects_on_one_engine_do_not_share_state(eng, cases, phasor):
    a, b = cases["t8_shared_flags"], cases["afsk1200_noise"]
    ma, mb, ta, tb = a.model(phasor), b.model(phasor), make(eng, a), make(eng, b)
    try:
        sa, sb = [s for s in a.steps if s[0] == "run"], [s for s in b.steps if s[0] == "run"]
        for i in range(max(len(sa), len(sb))):
            calls = []
            for t, m, st in ((ta, ma, sa), (tb, mb, sb)):
                if i < len(st):
                    call = DeviceCall(eng, t, st[i][1], st[i][2], st[i][3])
                    call.run()                                  # both queued before either is read
                    calls.append((call, m.run(st[i][1], st[i][2], st[i][3])))
            for call, want in calls:
                check(call.result(), want, i)
        assert [ta.state(c) for c in range(a.C)] == [ma.state(c) for c in range(a.C)]
        assert [tb.state(c) for c in range(b.C)] == [mb.state(c) for c in range(b.C)]
    finally:
        ta.close()
        tb.close()


def test_one_call_is_the_same_samples_in_two(eng, cases, phasor):
    case = cases["t8_shared_flags"]
    x = np.concatenate([s[1][:, :s[2]] for s in case.steps], axis=1)
    one, two = make(eng, case), make(eng, case)
    try:
        n1 = 333
        whole = run_device(eng, one, x, x.shape[1])
        first = run_device(eng, two, x[:, :n1].copy(), n1)
        second = run_device(eng, two, x[:, n1:].copy(), x.shape[1] - n1)
        assert np.array_equal(whole[0], first[0] + second[0]) and np.array_equal(whole[2], first[2] + second[2])
        assert fsk.frames_of(whole[2], whole[3], whole[4]) == sorted(fsk.frames_of(first[2], first[3], first[4]) +
                                                                     fsk.frames_of(second[2], second[3], second[4]))
        assert len(fsk.frames_of(whole[2], whole[3], whole[4])) == 6
        assert [one.state(c) for c in range(case.C)] == [two.state(c) for c in range(case.C)]
    finally:
        one.close()
        two.close()


def test_a_call_longer_than_the_walks_lds_chunk(eng, phasor):
    """the walk holds 65536 samples' decision words in LDS at a time: one call across that boundary, with frames back to back
    so that one straddles it, against the model; then the same stream again in two calls cut at the boundary"""
    cfg = dict(fc.T8, max_len=12)
    rng = np.random.default_rng(11)
    payloads = [bytes(rng.integers(0, 256, 8).astype(np.uint8)) for _ in range(100)]
    x = fc.audio(phasor, cfg, fm.hdlc_bits(payloads, 3, 1, 2))[None, :65536 + 600].astype(np.int16)
    n = x.shape[1]
    assert n == 65536 + 600
    m, t = fm.Model(1, phasor, **cfg), fsk.Fsk(eng, 1, **cfg)
    try:
        want = m.run(x, n)
        ends = want[3][0, :want[2][0]]["end_sample"]
        assert want[2][0] > 80 and (ends < 65536).any() and (ends > 65536).any()
        check(run_device(eng, t, x, n), want, "one call")
        assert t.state(0) == m.state(0)
        t.reset()
        first, second = run_device(eng, t, x[:, :65536].copy(), 65536), run_device(eng, t, x[:, 65536:].copy(), 600)
        assert first[2][0] + second[2][0] == want[2][0] and first[0][0] + second[0][0] == want[0][0]
        assert dict(t.state(0), samples=0) == dict(m.state(0), samples=0) and t.state(0)["samples"] == n
    finally:
        t.close()


def test_the_launch_count_is_the_headers_whatever_n_is(eng, cases, phasor):
    case = cases["t8_shared_flags"]
    t = make(eng, case)
    try:
        rng = np.random.default_rng(3)
        counts = {}
        for n in [0] + list(range(1, 40)) + [63, 64, 65, 255, 256, 257, 700, 5000]:
            call = DeviceCall(eng, t, rng.integers(-2000, 2000, (case.C, n + 1)).astype(np.int16), n, None)
            before = eng.stats()["device_launches"]
            call.run()
            counts[n] = eng.stats()["device_launches"] - before
            nb = call.result()[0]
            assert nb.max() <= 32 * t.max_bit_words(n)
        assert counts.pop(0) == 1 and set(counts.values()) == {LAUNCHES}, counts
    finally:
        t.close()
