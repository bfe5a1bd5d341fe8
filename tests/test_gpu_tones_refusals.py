"""GPU tier: every refusal of include/iqdemod_tones.h - the status, the argument's name in the message, which refusal wins
where two apply - and that a refusal queues nothing (device_launches and device_copies unchanged) and leaves the stream usable."""
import ctypes as C

import numpy as np
import pytest

from rtlsdrdiags_amd import capi, tones
from tests import tones_model as tm
from tests.addon_checks import EINVAL, eng, refused          # noqa: F401 (eng: a fixture)

pytestmark = pytest.mark.gpu

L, T, CH = 64, 3, 5
INCS = np.array([1 << 28, 1 << 29, 3 << 28], np.uint32)


CREATE = [
    (dict(abi_version=2), "abi_version"), (dict(abi_version=0), "abi_version"),
    (dict(n_channels=0), "n_channels"), (dict(n_channels=(1 << 20) + 1), "n_channels"),
    (dict(frame_len=0), "frame_len"), (dict(frame_len=16), "frame_len"), (dict(frame_len=48), "frame_len"), (dict(frame_len=8224), "frame_len"),
    (dict(ratio_q8=255), "ratio_q8"), (dict(ratio_q8=65536), "ratio_q8"), (dict(energy_q8=(1 << 20) + 1), "energy_q8"),
    (dict(open=0), "open"), (dict(open=256), "open"), (dict(hold=256), "hold"),
    (dict(reserved=(0, 0, 0, 1)), "reserved[3]"), (dict(reserved=(7, 0, 0, 0)), "reserved[0]"),
    # which wins: the header's order
    (dict(abi_version=3, n_channels=0), "abi_version"), (dict(n_channels=0, frame_len=1), "n_channels"),
    (dict(frame_len=1, ratio_q8=0), "frame_len"), (dict(ratio_q8=0, energy_q8=1 << 21), "ratio_q8"),
    (dict(energy_q8=1 << 21, open=0), "energy_q8"), (dict(open=0, hold=999), "open"), (dict(hold=999, reserved=(1, 0, 0, 0)), "hold"),
]


@pytest.mark.parametrize("over,word", CREATE, ids=[" ".join(o) for o, _ in CREATE])
def test_create_refuses(eng, over, word):
    kw = dict(n_channels=CH, phase_inc=INCS, frame_len=L)
    kw.update(over)
    n_channels, incs = kw.pop("n_channels"), kw.pop("phase_inc")
    refused(eng, lambda: tones.Tones(eng, n_channels, incs, **kw), "iqd_tones_create", word)


def test_create_refuses_tone_counts_pointers_and_the_window(eng):
    refused(eng, lambda: tones.Tones(eng, CH, np.zeros(0, np.uint32), frame_len=L), "n_tones")
    refused(eng, lambda: tones.Tones(eng, CH, np.zeros(65, np.uint32), frame_len=L), "n_tones")
    w = np.full(L, 32767, np.int16)
    w[17] = -32768
    refused(eng, lambda: tones.Tones(eng, CH, INCS, frame_len=L, window=w), "window[17]")
    refused(eng, lambda: tones.Tones(eng, CH, INCS, frame_len=L, window=w, ratio_q8=1), "window[17]")      # the window before the thresholds
    lib, h = tones._lib(), C.c_void_p()
    cfg = tones.TonesConfig(1, CH, L, T, INCS.ctypes.data, None, 0, 256, 0, 1, 0)
    assert lib.iqd_tones_create(None, C.byref(cfg), C.byref(h)) == EINVAL
    refused(eng, lambda: eng._check(lib.iqd_tones_create(eng._h, C.byref(cfg), None)), "out is NULL")
    refused(eng, lambda: eng._check(lib.iqd_tones_create(eng._h, None, None)), "out is NULL")                # out before cfg
    refused(eng, lambda: eng._check(lib.iqd_tones_create(eng._h, None, C.byref(h))), "cfg is NULL")
    cfg.phase_inc = None
    refused(eng, lambda: eng._check(lib.iqd_tones_create(eng._h, C.byref(cfg), C.byref(h))), "phase_inc is NULL")
    cfg.n_tones = 0
    refused(eng, lambda: eng._check(lib.iqd_tones_create(eng._h, C.byref(cfg), C.byref(h))), "n_tones")      # the count before the pointer
    assert not h.value


def test_run_refuses_and_the_stream_goes_on(eng):
    phasor = capi.channelizer_phasor_table()
    t = tones.Tones(eng, CH, INCS, frame_len=L, ratio_q8=256, open=1, hold=0)
    other = capi.Engine(n_channels=1)
    m = tm.Model(CH, L, INCS.tolist(), phasor)
    n, stride = 2 * L + 3, 2 * L + 8
    x = np.random.default_rng(5).integers(-30000, 30000, (CH, stride)).astype(np.int16)
    pcm, nf, fr, pw, cnt = (eng.dev_alloc(x.nbytes), eng.dev_alloc(64), eng.dev_alloc(CH * 3 * 40 + 64), eng.dev_alloc(CH * 3 * T * 8 + 64),
                            eng.dev_alloc(64))
    eng.dev_upload(pcm, x)
    eng.dev_upload(cnt, np.full(CH, n, np.uint32))
    try:
        good = dict(pcm_dev=pcm, row_stride=stride, n=n, n_frames_dev=nf, frames_dev=fr, power_dev=pw, count_dev=cnt)

        def dev(**over):
            return lambda: t.run_device(**dict(good, **over))

        who = "iqd_tones_run_device"
        refused(eng, dev(pcm_dev=0), who, "pcm is NULL")
        refused(eng, dev(n_frames_dev=0), who, "n_frames is NULL")
        refused(eng, dev(frames_dev=0), who, "frames is NULL")
        refused(eng, dev(n=stride + 1), who, "n (", "row_stride")
        refused(eng, dev(row_stride=1 << 31, n=5), who, "row_stride", "2^31 - 1")
        refused(eng, dev(pcm_dev=pcm + 1), who, "pcm_dev", "2-byte")
        refused(eng, dev(count_dev=cnt + 2), who, "count_dev", "4-byte")
        refused(eng, dev(n_frames_dev=nf + 2), who, "n_frames_dev", "4-byte")
        refused(eng, dev(frames_dev=fr + 8), who, "frames_dev", "16-byte")
        refused(eng, dev(power_dev=pw + 8), who, "power_dev", "16-byte")
        # which wins
        refused(eng, dev(pcm_dev=0, frames_dev=0), who, "pcm is NULL")
        refused(eng, dev(n_frames_dev=0, frames_dev=0), who, "n_frames is NULL")
        refused(eng, dev(frames_dev=0, n=stride + 1), who, "frames is NULL")                  # NULLs before counts
        refused(eng, dev(n=(1 << 31) + 5, row_stride=1 << 31), who, "n (")                    # n before row_stride
        refused(eng, dev(n=stride + 1, frames_dev=fr + 8), who, "n (")                        # counts before alignment
        refused(eng, dev(pcm_dev=pcm + 1, frames_dev=fr + 8), who, "pcm_dev")                 # alignment in argument order
        refused(eng, dev(frames_dev=fr + 8, power_dev=pw + 8), who, "frames_dev")
        # another engine's object: before everything else; the text is left with the object's engine
        before = other.stats()["device_launches"]
        refused(eng, dev(engine=other, pcm_dev=0), who, "another engine")
        assert other.stats()["device_launches"] == before

        host_nf, host_fr = np.zeros(CH, np.uint32), np.zeros((CH, 3), tones.TONES_FRAME)
        lib = tones._lib()

        def host(pcm_=x, stride_=stride, n_=n, nf_=host_nf, fr_=host_fr, e_=eng):
            return lambda: eng._check(lib.iqd_tones_run(e_._h, t._h, capi._np_ptr(pcm_), stride_, None, n_, capi._np_ptr(nf_), capi._np_ptr(fr_), None))

        refused(eng, host(pcm_=None), "iqd_tones_run:", "pcm is NULL")
        refused(eng, host(nf_=None), "iqd_tones_run:", "n_frames is NULL")
        refused(eng, host(fr_=None, n_=stride + 1), "iqd_tones_run:", "frames is NULL")
        refused(eng, host(n_=stride + 1), "iqd_tones_run:", "n (")
        refused(eng, host(e_=other), "iqd_tones_run:", "another engine")
        assert lib.iqd_tones_run_device(eng._h, None, None, 0, None, 0, None, None, None) == EINVAL
        assert lib.iqd_tones_reset(None) == EINVAL and lib.iqd_tones_get_state(None, 0, None) == EINVAL
        refused(eng, lambda: t.state(CH), "iqd_tones_get_state", "channel")
        refused(eng, lambda: eng._check(lib.iqd_tones_get_state(t._h, 0, None)), "iqd_tones_get_state", "state is NULL")

        # nothing moved: the object is as created, and the stream runs the good call
        assert t.state(0) == dict(tone=-1, cand=-1, run=0, miss=0, fill=0)
        t.run_device(**good)
        eng.synchronize()
        want = m.run(x, n, None)
        assert np.array_equal(eng.dev_download(nf, CH * 4, np.uint32), want[0])
        assert eng.dev_download(fr, CH * 3 * 40).tobytes() == want[1].tobytes()
        assert np.array_equal(eng.dev_download(pw, CH * 3 * T * 8, np.uint64).reshape(CH, 3, T), want[2])
    finally:
        t.close()
        other.close()
        for p in (pcm, nf, fr, pw, cnt):
            eng.dev_free(p)
