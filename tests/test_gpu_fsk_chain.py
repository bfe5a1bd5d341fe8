"""GPU tier: the packet decoder behind the FM chain on one stream.  An FM carrier modulated by one AFSK frame (tests/fsk_cases.py:
chain_iq; tests/test_fsk_host.py shows that the oracle's PCM alone decodes to the payload) goes, the same on 3 channels, through
Engine.set_mode("fm") + accept_device and Fsk.run_device on the PCM rows and counts the accept leaves on the device, block by
block with no synchronise in between, and is compared bit for bit with tests/fsk_model.py run on the engine's PCM."""
import numpy as np
import pytest

from rtlsdrdiags_amd import capi, fsk
from tests import fsk_cases as fc
from tests import fsk_model as fm

pytestmark = pytest.mark.gpu
CH = 3


def test_afsk_behind_the_fm_accept_on_one_stream(oracle):
    phasor = capi.channelizer_phasor_table()
    iq = fc.chain_iq()
    chain = oracle.chain()
    chain.set_mode("fm")
    ref_pcm, _, _ = chain.accept_stream(iq)
    block = 32768
    calls, n = len(iq) // block, block // 64                     # 512 PCM samples of a block of 32768 bytes
    assert len(iq) % block == 0 and len(ref_pcm) == calls * n and calls >= 2
    cfg = fsk.afsk1200(8000)
    assert cfg == fm.afsk1200(8000)
    m = fm.Model(CH, phasor, **cfg)

    eng = capi.Engine(n_channels=CH)
    t = fsk.Fsk(eng, CH, **cfg)
    F, Bw, Bc = t.max_frames(n), t.max_bit_words(n), t.max_bytes(n)
    iq_d, pcm_d, cnt_d = eng.dev_alloc(calls * CH * block), eng.dev_alloc(calls * CH * n * 2), eng.dev_alloc(calls * 16)
    nb_d, nf_d = eng.dev_alloc(calls * 16), eng.dev_alloc(calls * 16)
    bits_d, fr_d, by_d = eng.dev_alloc(calls * CH * Bw * 4), eng.dev_alloc(calls * CH * F * 24 + 16), eng.dev_alloc(calls * CH * Bc)
    try:
        eng.set_mode("fm")
        eng.dev_upload(iq_d, np.concatenate([np.tile(iq[k * block:(k + 1) * block], CH) for k in range(calls)]))
        for k in range(calls):                                   # every call's arrays in their own place; nothing waits in between
            eng.accept_device(iq_d + k * CH * block, block, pcm_d + k * CH * n * 2, cnt_d + k * 16)
            t.run_device(pcm_d + k * CH * n * 2, n, n, nb_d + k * 16, nf_d + k * 16, fr_d + k * CH * F * 24, by_d + k * CH * Bc,
                         bits_dev=bits_d + k * CH * Bw * 4, count_dev=cnt_d + k * 16)
        eng.synchronize()
        pcm = eng.dev_download(pcm_d, calls * CH * n * 2, np.int16).reshape(calls, CH, n)
        for c in range(CH):
            assert np.array_equal(pcm[:, c].reshape(-1), ref_pcm), c
        found = []
        for k in range(calls):
            cnt = eng.dev_download(cnt_d + k * 16, CH * 4, np.uint32)
            assert (cnt == n).all()
            want = m.run(pcm[k], n, cnt)
            assert np.array_equal(eng.dev_download(nb_d + k * 16, CH * 4, np.uint32), want[0]), k
            assert np.array_equal(eng.dev_download(bits_d + k * CH * Bw * 4, CH * Bw * 4, np.uint32).reshape(CH, Bw), want[1]), k
            assert np.array_equal(eng.dev_download(nf_d + k * 16, CH * 4, np.uint32), want[2]), k
            assert eng.dev_download(fr_d + k * CH * F * 24, CH * F * 24).tobytes() == want[3].tobytes(), k
            assert np.array_equal(eng.dev_download(by_d + k * CH * Bc, CH * Bc, np.uint8).reshape(CH, Bc), want[4]), k
            found += fsk.frames_of(want[2], want[3], want[4])
        assert sorted(c for c, _, _, _ in found) == list(range(CH)) and all(p == fc.chain_payload() for _, _, p, _ in found), found
        for c in range(CH):
            assert t.state(c) == m.state(c) and t.state(c)["frames_total"] == 1 and t.state(c)["bad_fcs"] == 0
    finally:
        t.close()
        for p in (iq_d, pcm_d, cnt_d, nb_d, nf_d, bits_d, fr_d, by_d):
            eng.dev_free(p)
        eng.close()
