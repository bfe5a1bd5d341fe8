"""GPU tier of the PCM tone bank (include/iqdemod_tones.h): every case of tests/tones_cases.py bit for bit against
tests/tones_model.py - n_frames, every record, every power row, the zero tail, get_state - through run_device on rows that are
only 2-byte aligned and on output arrays filled with another value beforehand; then run against run_device, power_dev = NULL,
two objects on one engine, one call against the same samples in two, and the launch count."""
import numpy as np
import pytest

from rtlsdrdiags_amd import capi, tones
from tests import tones_cases as tc
from tests import tones_model as tm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def phasor():
    return capi.channelizer_phasor_table()


@pytest.fixture(scope="module")
def cases(phasor):
    return {c.name: c for c in tc.build(phasor)}


@pytest.fixture(scope="module")
def eng():
    e = capi.Engine(n_channels=1)
    yield e
    e.close()


def make(eng, case, **over):
    return tones.Tones(eng, case.C, np.array(case.incs, np.uint32), frame_len=case.L, window=case.window, **dict(case.thresholds, **over))


class DeviceCall:
    """one run_device call's arrays on the device: the rows from 2 bytes behind an aligned address on, the outputs filled with
    0xAB bytes"""

    def __init__(self, eng, t, pcm, n, count, want_power=True):
        self.eng, self.t = eng, t
        C, stride = pcm.shape
        self.C, self.F, self.T = C, t.max_frames(n), t.n_tones
        self.ptrs = []
        self.pcm = self._put(np.concatenate([np.zeros(1, np.int16), pcm.reshape(-1)])) + 2
        self.count = self._put(np.ascontiguousarray(count, np.uint32)) if count is not None else 0
        self.nf = self._put(np.full(C * 4, 0xAB, np.uint8))
        self.frames = self._put(np.full(max(C * self.F * 40, 16), 0xAB, np.uint8))
        self.power = self._put(np.full(max(C * self.F * self.T * 8, 16), 0xAB, np.uint8)) if want_power else 0
        self.stride, self.n = stride, n

    def _put(self, a):
        p = self.eng.dev_alloc(max(a.nbytes, 16))
        self.ptrs.append(p)
        self.eng.dev_upload(p, a)
        return p

    def run(self):
        self.t.run_device(self.pcm, self.stride, self.n, self.nf, self.frames, power_dev=self.power, count_dev=self.count)

    def result(self):
        """(n_frames, frames, power or None); synchronises, frees"""
        self.eng.synchronize()
        nf = self.eng.dev_download(self.nf, self.C * 4, np.uint32)
        frames = np.zeros((self.C, self.F), tones.TONES_FRAME)
        power = np.zeros((self.C, self.F, self.T), np.uint64) if self.power else None
        if self.F:
            frames = self.eng.dev_download(self.frames, self.C * self.F * 40, np.uint8).view(tones.TONES_FRAME).reshape(self.C, self.F)
            if self.power:
                power = self.eng.dev_download(self.power, self.C * self.F * self.T * 8, np.uint64).reshape(self.C, self.F, self.T)
        for p in self.ptrs:
            self.eng.dev_free(p)
        return nf, frames, power


def run_device(eng, t, pcm, n, count=None, want_power=True):
    call = DeviceCall(eng, t, pcm, n, count, want_power)
    call.run()
    return call.result()


def check(got, want, what):
    nf, frames, power = got
    assert np.array_equal(nf, want[0]), (what, nf, want[0])
    for k in tm.FRAME.names:
        assert np.array_equal(frames[k], want[1][k]), (what, k, frames[k], want[1][k])
    assert frames.tobytes() == want[1].tobytes(), what
    if power is not None:
        assert np.array_equal(power, want[2]), what


@pytest.mark.parametrize("name", list(tc.BLIND))
def test_corpus_case_bit_for_bit(eng, cases, phasor, name):
    case = cases[name]
    m, t = case.model(phasor), make(eng, case)
    try:
        assert t.state(case.C - 1) == dict(tone=-1, cand=-1, run=0, miss=0, fill=0)
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


@pytest.mark.parametrize("name", ["l64_t15_c15_counts", "l32_t17_c17_cuts", "alternating_t1"])
def test_run_is_run_device(eng, cases, phasor, name):
    case = cases[name]
    m, t = case.model(phasor), make(eng, case)
    try:
        for i, s in enumerate(case.steps):
            check(t.run(s[1], s[2], s[3]), m.run(s[1], s[2], s[3]), (name, i))
        assert [t.state(c) for c in range(case.C)] == [m.state(c) for c in range(case.C)]
    finally:
        t.close()


def test_without_power_the_records_are_the_same(eng, cases, phasor):
    case = cases["l96_t16_c16"]
    m, t = case.model(phasor), make(eng, case)
    try:
        for i, s in enumerate(case.steps):
            got = run_device(eng, t, s[1], s[2], s[3], want_power=False)
            assert got[2] is None
            check(got, m.run(s[1], s[2], s[3]), i)
        s = case.steps[-1]
        host = t.run(s[1], s[2], s[3], want_power=False)
        assert host[2] is None
        check(host, m.run(s[1], s[2], s[3]), "host")
    finally:
        t.close()


def test_two_objects_on_one_engine_do_not_share_state(eng, cases, phasor):
    a, b = cases["decision_open2_hold1"], cases["reset_in_mid_frame"]
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
        assert ta.state(0) == ma.state(0) and [tb.state(c) for c in range(b.C)] == [mb.state(c) for c in range(b.C)]
    finally:
        ta.close()
        tb.close()


def test_one_call_is_the_same_samples_in_two(eng, cases, phasor):
    case = cases["l96_t16_c16"]
    x = np.concatenate([s[1][:, :s[2]] for s in case.steps], axis=1)
    one, two = make(eng, case), make(eng, case)
    try:
        n1 = 3 * case.L + 5
        whole = run_device(eng, one, x, x.shape[1])
        first = run_device(eng, two, x[:, :n1].copy(), n1)
        second = run_device(eng, two, x[:, n1:].copy(), x.shape[1] - n1)
        k1 = int(first[0][0])
        assert (first[0] == k1).all() and np.array_equal(whole[0], first[0] + second[0])
        k = int(whole[0][0])
        assert whole[1][:, :k].tobytes() == np.concatenate([first[1][:, :k1], second[1][:, :k - k1]], axis=1).tobytes()
        assert np.array_equal(whole[2][:, :k], np.concatenate([first[2][:, :k1], second[2][:, :k - k1]], axis=1))
        assert [one.state(c) for c in range(case.C)] == [two.state(c) for c in range(case.C)]
    finally:
        one.close()
        two.close()


def test_the_launch_count_does_not_grow_with_n(eng, cases, phasor):
    case = cases["l32_t17_c17_cuts"]
    t = make(eng, case)
    try:
        rng = np.random.default_rng(3)
        counts = {}
        for n in (0, 1, case.L, 3 * case.L + 5, 400 * case.L + 7):
            call = DeviceCall(eng, t, rng.integers(-2000, 2000, (case.C, n + 1)).astype(np.int16), n, None)
            before = eng.stats()["device_launches"]
            call.run()
            counts[n] = eng.stats()["device_launches"] - before
            nf = call.result()[0]
            assert nf.max() <= t.max_frames(n)
        assert counts.pop(0) == 1 and set(counts.values()) == {2}, counts
    finally:
        t.close()
