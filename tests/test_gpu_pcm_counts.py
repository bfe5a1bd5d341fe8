"""GPU tier: what a call of the two PCM add-ons (include/iqdemod_tones.h, include/iqdemod_fsk.h) queues - the launches and the
copies Engine.stats() counts - in every form: the host run with and without the arrays the caller may leave out, an empty
call, run_device, reset and get_state.  The figures are read off the host code: a copy per array that is given and not empty,
a launch less where n is 0."""
import numpy as np
import pytest

from rtlsdrdiags_amd import fsk, tones
from tests import fsk_cases as fc
from tests.addon_checks import eng          # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

CH, STRIDE, N = 3, 48, 40
#            host run, all given   none given   n = 0, all given   run_device   reset    state(0)
WANT = {"tones": [(2, 5),          (2, 3),      (1, 3),            (2, 0),      (1, 0),  (0, 1)],
        "fsk":   [(2, 7),          (2, 5),      (1, 4),            (2, 0),      (0, 2),  (0, 1)]}


def queued(eng, fn):
    before = eng.stats()
    fn()
    after = eng.stats()
    return after["device_launches"] - before["device_launches"], after["device_copies"] - before["device_copies"]


@pytest.mark.parametrize("kind", ["tones", "fsk"])
def test_what_every_call_queues(eng, kind):
    pcm = np.random.default_rng(7).integers(-20000, 20000, (CH, STRIDE)).astype(np.int16)
    count = np.array([N, 0, N - 7], np.uint32)
    if kind == "tones":
        t = tones.Tones(eng, CH, np.array([1 << 28, 1 << 29, 3 << 28], np.uint32), frame_len=32)
        optional, sizes = "want_power", [CH * 4, CH * t.max_frames(N) * 40, CH * t.max_frames(N) * 3 * 8]
    else:
        t = fsk.Fsk(eng, CH, **fc.T8)
        optional, sizes = "want_bits", [CH * 4, CH * 4, CH * t.max_frames(N) * 24, CH * t.max_bytes(N), CH * t.max_bit_words(N) * 4]
    ptrs = [eng.dev_alloc(pcm.nbytes)] + [eng.dev_alloc(s + 16) for s in sizes]
    eng.dev_upload(ptrs[0], pcm)
    try:
        if kind == "tones":
            device = lambda: t.run_device(ptrs[0], STRIDE, N, ptrs[1], ptrs[2], power_dev=ptrs[3])
        else:
            device = lambda: t.run_device(ptrs[0], STRIDE, N, ptrs[1], ptrs[2], ptrs[3], ptrs[4], bits_dev=ptrs[5])
        calls = [lambda: t.run(pcm, N, count, **{optional: True}), lambda: t.run(pcm, N, None, **{optional: False}),
                 lambda: t.run(pcm, 0, count, **{optional: True}), device, t.reset, lambda: t.state(0)]
        got = [queued(eng, c) for c in calls]
        assert got == WANT[kind]
    finally:
        eng.synchronize()
        t.close()
        for p in ptrs:
            eng.dev_free(p)
