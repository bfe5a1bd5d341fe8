"""GPU tier: the tone bank behind the FM chain on one stream.  A synthetic FM signal carrying a CTCSS tone under a 1 kHz audio
tone (tests/tones_cases.py: chain_iq; tests/test_tones_host.py shows that the oracle's PCM alone names the tone) goes through
Engine.set_mode("fm") + accept_device and Tones.run_device on the PCM rows and counts the accept leaves on the device, with no
synchronise in between, and is compared bit for bit with tests/tones_model.py run on the oracle's PCM."""
import numpy as np
import pytest

from rtlsdrdiags_amd import capi, tones
from tests import tones_cases as tc
from tests import tones_model as tm

pytestmark = pytest.mark.gpu


def test_ctcss_behind_the_fm_accept_on_one_stream(oracle):
    phasor = capi.channelizer_phasor_table()
    iq = tc.chain_iq()
    chain = oracle.chain()
    chain.set_mode("fm")
    ref_pcm, _, _ = chain.accept_stream(iq)
    incs = [tones.phase_inc(f, tc.PCM_RATE) for f in tones.ctcss_mhz()]
    cfg = {k: v for k, v in tones.CTCSS_DEFAULTS.items() if k != "frame_len"}
    m = tm.Model(1, 4096, incs, phasor, **cfg)

    # two calls of one and a half frames each: the second completes a frame begun in the first
    half = len(iq) // 2
    n = half // 64
    assert half % 32768 == 0 and len(ref_pcm) == 2 * n and n == 4096 * 3 // 2
    eng = capi.Engine(n_channels=1)
    t = tones.Tones(eng, 1, np.array(incs, np.uint32), frame_len=4096, **cfg)
    F = t.max_frames(n)
    iq_d, pcm_d, cnt_d = eng.dev_alloc(len(iq)), eng.dev_alloc(2 * n * 2), eng.dev_alloc(2 * 16)
    nf_d, fr_d, pw_d = eng.dev_alloc(2 * 16), eng.dev_alloc(2 * F * 40 + 16), eng.dev_alloc(2 * F * 50 * 8)
    try:
        eng.set_mode("fm")
        eng.dev_upload(iq_d, iq)
        fr_call = (F * 40 + 15) // 16 * 16
        for k in range(2):                                       # every call's outputs in their own place; nothing waits in between
            eng.accept_device(iq_d + k * half, half, pcm_d + k * n * 2, cnt_d + k * 16)
            t.run_device(pcm_d + k * n * 2, n, n, nf_d + k * 16, fr_d + k * fr_call, power_dev=pw_d + k * F * 50 * 8, count_dev=cnt_d + k * 16)
        eng.synchronize()
        pcm = eng.dev_download(pcm_d, 2 * n * 2, np.int16)
        assert np.array_equal(pcm, ref_pcm)
        total = []
        for k in range(2):
            want = m.run(ref_pcm[None, k * n:(k + 1) * n], n, np.array([n], np.uint32))
            assert eng.dev_download(cnt_d + k * 16, 4, np.uint32)[0] == n
            assert np.array_equal(eng.dev_download(nf_d + k * 16, 4, np.uint32), want[0])
            assert eng.dev_download(fr_d + k * fr_call, F * 40).tobytes() == want[1].tobytes(), k
            assert np.array_equal(eng.dev_download(pw_d + k * F * 50 * 8, F * 50 * 8, np.uint64).reshape(1, F, 50), want[2])
            total += [r for r in want[1][0, :int(want[0][0])]]
        assert len(total) == tc.CHAIN_FRAMES and all(r["best"] == tc.CHAIN_TONE for r in total)
        assert [int(r["tone"]) for r in total] == [-1, tc.CHAIN_TONE, tc.CHAIN_TONE] and total[1]["flags"] == tm.F_OPENED
        assert t.state(0) == m.state(0) == dict(tone=tc.CHAIN_TONE, cand=tc.CHAIN_TONE, run=3, miss=0, fill=0)
    finally:
        t.close()
        for p in (iq_d, pcm_d, cnt_d, nf_d, fr_d, pw_d):
            eng.dev_free(p)
        eng.close()
