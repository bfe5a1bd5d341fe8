"""GPU tier: every refusal of include/iqdemod_fsk.h - the status, the argument's name in the message, which refusal wins where
two apply - and that a refusal queues nothing (device_launches and device_copies unchanged) and leaves the stream usable."""
import ctypes as C

import numpy as np
import pytest

from rtlsdrdiags_amd import capi, fsk
from tests import fsk_cases as fc
from tests import fsk_model as fm
from tests.addon_checks import EINVAL, eng, refused          # noqa: F401 (eng: a fixture)

pytestmark = pytest.mark.gpu

CH = 5
GOOD = dict(fc.T8)


CREATE = [
    (dict(abi_version=2), "abi_version"), (dict(abi_version=0), "abi_version"),
    (dict(n_channels=0), "n_channels"), (dict(n_channels=(1 << 20) + 1), "n_channels"),
    (dict(corr_len=0), "corr_len"), (dict(corr_len=1), "corr_len"), (dict(corr_len=65), "corr_len"),
    (dict(baud_inc=(1 << 20) - 1), "baud_inc"), (dict(baud_inc=1 << 31), "baud_inc"), (dict(baud_inc=0), "baud_inc"),
    (dict(loop_shift=0), "loop_shift"), (dict(loop_shift=9), "loop_shift"),
    (dict(flags=2), "flags"), (dict(flags=3), "flags"), (dict(flags=1 << 31), "flags"),
    (dict(min_len=2), "min_len"), (dict(min_len=9, max_len=8), "min_len"), (dict(max_len=1025), "max_len"),
    (dict(reserved=(0, 0, 0, 1)), "reserved[3]"), (dict(reserved=(7, 0, 0, 0)), "reserved[0]"),
    # which wins: the header's order
    (dict(abi_version=3, n_channels=0), "abi_version"), (dict(n_channels=0, corr_len=1), "n_channels"),
    (dict(corr_len=1, baud_inc=0), "corr_len"), (dict(baud_inc=0, loop_shift=0), "baud_inc"), (dict(loop_shift=0, flags=2), "loop_shift"),
    (dict(flags=2, min_len=0), "flags"), (dict(min_len=0, max_len=2000), "min_len"), (dict(max_len=2000, reserved=(1, 0, 0, 0)), "max_len"),
]


@pytest.mark.parametrize("over,word", CREATE, ids=[" ".join(o) for o, _ in CREATE])
def test_create_refuses(eng, over, word):
    kw = dict(GOOD, n_channels=CH)
    kw.update(over)
    n_channels = kw.pop("n_channels")
    refused(eng, lambda: fsk.Fsk(eng, n_channels, **kw), "iqd_fsk_create", word)


def test_create_refuses_the_window_and_pointers(eng):
    for bad in (32513, -32513, 32767, -32768):
        w = np.full(8, 32512, np.int16)
        w[5] = bad
        refused(eng, lambda: fsk.Fsk(eng, CH, window=w, **GOOD), "window[5]")
        refused(eng, lambda: fsk.Fsk(eng, CH, window=w, **dict(GOOD, min_len=0)), "window[5]")       # the window before the lengths
        refused(eng, lambda: fsk.Fsk(eng, CH, window=w, **dict(GOOD, flags=4)), "flags")             # and behind the flags
    lib, h = fsk._lib(), C.c_void_p()
    cfg = fsk.FskConfig(1, CH, 8, 1 << 29, 1 << 30, 1 << 29, 3, 1, None, 3, 8)
    assert lib.iqd_fsk_create(None, C.byref(cfg), C.byref(h)) == EINVAL
    refused(eng, lambda: eng._check(lib.iqd_fsk_create(eng._h, C.byref(cfg), None)), "out is NULL")
    refused(eng, lambda: eng._check(lib.iqd_fsk_create(eng._h, None, None)), "out is NULL")                # out before cfg
    refused(eng, lambda: eng._check(lib.iqd_fsk_create(eng._h, None, C.byref(h))), "cfg is NULL")
    assert not h.value


def test_run_refuses_and_the_stream_goes_on(eng):
    phasor = capi.channelizer_phasor_table()
    t = fsk.Fsk(eng, CH, **GOOD)
    other = capi.Engine(n_channels=1)
    m = fm.Model(CH, phasor, **GOOD)
    case = next(c for c in fc.build(phasor) if c.name == "t8_shared_flags")
    row = np.concatenate([s[1][0, :s[2]] for s in case.steps])
    n, stride = len(row), len(row) + 8
    x = np.zeros((CH, stride), np.int16)
    x[:, :n] = row
    F, Bw, Bc = t.max_frames(n), t.max_bit_words(n), t.max_bytes(n)
    pcm, cnt, nb, nf = eng.dev_alloc(x.nbytes), eng.dev_alloc(64), eng.dev_alloc(64), eng.dev_alloc(64)
    bits, fr, by = eng.dev_alloc(CH * Bw * 4 + 64), eng.dev_alloc(CH * F * 24 + 64), eng.dev_alloc(CH * Bc + 64)
    eng.dev_upload(pcm, x)
    eng.dev_upload(cnt, np.full(CH, n, np.uint32))
    try:
        good = dict(pcm_dev=pcm, row_stride=stride, n=n, n_bits_dev=nb, n_frames_dev=nf, frames_dev=fr, bytes_dev=by, bits_dev=bits, count_dev=cnt)

        def dev(**over):
            return lambda: t.run_device(**dict(good, **over))

        who = "iqd_fsk_run_device"
        refused(eng, dev(pcm_dev=0), who, "pcm is NULL")
        refused(eng, dev(n_bits_dev=0), who, "n_bits is NULL")
        refused(eng, dev(n_frames_dev=0), who, "n_frames is NULL")
        refused(eng, dev(frames_dev=0), who, "frames is NULL")
        refused(eng, dev(bytes_dev=0), who, "bytes is NULL")
        refused(eng, dev(n=stride + 1), who, "n (", "row_stride")
        refused(eng, dev(row_stride=1 << 31, n=5), who, "row_stride", "2^31 - 1")
        refused(eng, dev(pcm_dev=pcm + 1), who, "pcm_dev", "2-byte")
        refused(eng, dev(count_dev=cnt + 2), who, "count_dev", "4-byte")
        refused(eng, dev(n_bits_dev=nb + 2), who, "n_bits_dev", "4-byte")
        refused(eng, dev(bits_dev=bits + 2), who, "bits_dev", "4-byte")
        refused(eng, dev(n_frames_dev=nf + 2), who, "n_frames_dev", "4-byte")
        refused(eng, dev(frames_dev=fr + 4), who, "frames_dev", "8-byte")
        refused(eng, dev(bytes_dev=by + 8), who, "bytes_dev", "16-byte")
        # which wins
        refused(eng, dev(pcm_dev=0, frames_dev=0), who, "pcm is NULL")
        refused(eng, dev(n_bits_dev=0, n_frames_dev=0), who, "n_bits is NULL")
        refused(eng, dev(n_frames_dev=0, frames_dev=0), who, "n_frames is NULL")
        refused(eng, dev(frames_dev=0, bytes_dev=0), who, "frames is NULL")
        refused(eng, dev(bytes_dev=0, n=stride + 1), who, "bytes is NULL")                    # NULLs before counts
        refused(eng, dev(n=(1 << 31) + 5, row_stride=1 << 31), who, "n (")                    # n before row_stride
        refused(eng, dev(n=stride + 1, frames_dev=fr + 4), who, "n (")                        # counts before alignment
        refused(eng, dev(pcm_dev=pcm + 1, frames_dev=fr + 4), who, "pcm_dev")                 # alignment in argument order
        refused(eng, dev(bits_dev=bits + 2, n_frames_dev=nf + 2), who, "bits_dev")
        refused(eng, dev(frames_dev=fr + 4, bytes_dev=by + 8), who, "frames_dev")
        # another engine's object: before everything else; the text is left with the object's engine
        before = other.stats()["device_launches"]
        refused(eng, dev(engine=other, pcm_dev=0), who, "another engine")
        assert other.stats()["device_launches"] == before

        host = dict(pcm=x, nb=np.zeros(CH, np.uint32), nf=np.zeros(CH, np.uint32), fr=np.zeros((CH, F), fsk.FSK_FRAME),
                    by=np.zeros((CH, Bc), np.uint8))
        lib = fsk._lib()

        def run(e_=eng, stride_=stride, n_=n, **over):
            a = dict(host, **over)
            return lambda: eng._check(lib.iqd_fsk_run(e_._h, t._h, capi._np_ptr(a["pcm"]), stride_, None, n_, capi._np_ptr(a["nb"]), None,
                                                      capi._np_ptr(a["nf"]), capi._np_ptr(a["fr"]), capi._np_ptr(a["by"])))

        refused(eng, run(pcm=None), "iqd_fsk_run:", "pcm is NULL")
        refused(eng, run(nb=None), "iqd_fsk_run:", "n_bits is NULL")
        refused(eng, run(nf=None), "iqd_fsk_run:", "n_frames is NULL")
        refused(eng, run(fr=None, n_=stride + 1), "iqd_fsk_run:", "frames is NULL")
        refused(eng, run(by=None), "iqd_fsk_run:", "bytes is NULL")
        refused(eng, run(n_=stride + 1), "iqd_fsk_run:", "n (")
        refused(eng, run(e_=other), "iqd_fsk_run:", "another engine")
        assert lib.iqd_fsk_run_device(eng._h, None, None, 0, None, 0, None, None, None, None, None) == EINVAL
        assert lib.iqd_fsk_run(eng._h, None, None, 0, None, 0, None, None, None, None, None) == EINVAL
        assert lib.iqd_fsk_reset(None) == EINVAL and lib.iqd_fsk_get_state(None, 0, None) == EINVAL
        refused(eng, lambda: t.state(CH), "iqd_fsk_get_state", "channel")
        refused(eng, lambda: eng._check(lib.iqd_fsk_get_state(t._h, 0, None)), "iqd_fsk_get_state", "state is NULL")

        # nothing moved: the object is as created, and the stream runs the good call
        assert t.state(0) == dict(samples=0, ph=0, prev=0, last=0, ones=0, in_frame=0, nbits=0, bad_fcs=0, frames_total=0)
        t.run_device(**good)
        eng.synchronize()
        want = m.run(x, n, None)
        assert want[2].tolist() == [3] * CH
        assert np.array_equal(eng.dev_download(nb, CH * 4, np.uint32), want[0])
        assert np.array_equal(eng.dev_download(bits, CH * Bw * 4, np.uint32).reshape(CH, Bw), want[1])
        assert np.array_equal(eng.dev_download(nf, CH * 4, np.uint32), want[2])
        assert eng.dev_download(fr, CH * F * 24).tobytes() == want[3].tobytes()
        assert np.array_equal(eng.dev_download(by, CH * Bc, np.uint8).reshape(CH, Bc), want[4])
    finally:
        t.close()
        other.close()
        for p in (pcm, cnt, nb, nf, bits, fr, by):
            eng.dev_free(p)
