"""The PCM packet decoder of libiqdemod.so (include/iqdemod_fsk.h: iqd_fsk_*): the audio-FSK bits (Bell 202: APRS / AX.25
packet) and the HDLC frames in every channel's PCM, on the engine's stream.  An add-on like tones.py: its functions have their
own table here, which capi._bind sets on the loaded library at first use; capi.PROTOTYPES is include/iqdemod.h alone."""
import ctypes as C

import numpy as np

from . import capi
from .capi import IqdError, _dev_ptr, _np_ptr, _ok

ABI_VERSION = 1
NRZI = 1


class FskConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_channels", C.c_uint32), ("corr_len", C.c_uint32), ("mark_inc", C.c_uint32),
                ("space_inc", C.c_uint32), ("baud_inc", C.c_uint32), ("loop_shift", C.c_uint32), ("flags", C.c_uint32),
                ("window", C.c_void_p), ("min_len", C.c_uint32), ("max_len", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class FskState(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("ph", C.c_uint32), ("prev", C.c_uint32), ("last", C.c_uint32), ("ones", C.c_uint32),
                ("in_frame", C.c_uint32), ("nbits", C.c_uint32), ("bad_fcs", C.c_uint32), ("frames_total", C.c_uint32)]


FSK_FRAME = np.dtype([("end_sample", "<u8"), ("offset", "<u4"), ("len", "<u4"), ("fcs", "<u4"), ("flags", "<u4")])

_vp, _u32, _u64, _sz, _int, _P = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int, C.POINTER

# Every function of include/iqdemod_fsk.h, in its order: name -> (what it returns, what it takes), as capi.PROTOTYPES.
# tests/test_fsk_host.py holds this against the header.
PROTOTYPES = {
    "iqd_fsk_create": (_int, (_vp, _P(FskConfig), _P(_vp))),
    "iqd_fsk_destroy": (None, (_vp,)),
    "iqd_fsk_reset": (_int, (_vp,)),
    "iqd_fsk_max_frames": (_sz, (_vp, _sz)),
    "iqd_fsk_max_bit_words": (_sz, (_vp, _sz)),
    "iqd_fsk_max_bytes": (_sz, (_vp, _sz)),
    "iqd_fsk_run_device": (_int, (_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp)),
    "iqd_fsk_run": (_int, (_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp, _vp, _vp)),
    "iqd_fsk_get_state": (_int, (_vp, _u32, _P(FskState))),
    "iqd_fsk_phase_inc": (_int, (_u64, _u32, _P(_u32))),
    "iqd_fsk_afsk1200": (_int, (_u32, _P(FskConfig))),
}


def _lib():
    """capi's library with this table's prototypes set (once)"""
    return capi._addon_lib(PROTOTYPES)


def phase_inc(freq_mhz, rate_hz):
    """iqd_fsk_phase_inc (host only): a tone's phase increment from its frequency in millihertz (a bit clock's from the baud
    rate in thousandths) and the PCM rate in Hz"""
    return capi._addon_phase_inc(PROTOTYPES, "fsk", freq_mhz, rate_hz)


def afsk1200(rate_hz):
    """iqd_fsk_afsk1200 (host only): Fsk's keyword arguments for Bell 202 packet at a PCM rate - 1200 / 2200 Hz, 1200 baud,
    corr_len 8, loop_shift 3, NRZI, min_len 17, max_len 512"""
    cfg = FskConfig()
    if not 0 <= int(rate_hz) <= 0xffffffff:
        raise IqdError(-1, "iqd_fsk_afsk1200: rate_hz %r out of range" % (rate_hz,))
    _ok(_lib().iqd_fsk_afsk1200(int(rate_hz), C.byref(cfg)), "iqd_fsk_afsk1200: no Bell 202 increments at rate_hz %r" % (rate_hz,))
    return dict(corr_len=cfg.corr_len, mark_inc=cfg.mark_inc, space_inc=cfg.space_inc, baud_inc=cfg.baud_inc, loop_shift=cfg.loop_shift,
                flags=cfg.flags, min_len=cfg.min_len, max_len=cfg.max_len)


class Fsk(capi._PcmChild):
    """iqd_fsk_*: per channel the decisions of two corr_len-tap tone correlators, a bit clock that follows their transitions,
    NRZI and an HDLC deframer with the CRC-16/X.25 check; a call gives the bits and the good frames it completed.  State is
    carried from call to call until reset().  state(channel): dict(samples, ph, prev, last, ones, in_frame, nbits, bad_fcs,
    frames_total)."""
    _State = FskState

    def __init__(self, engine, n_channels, mark_inc, space_inc, baud_inc, corr_len=8, loop_shift=3, flags=NRZI, window=None, min_len=17,
                 max_len=512, reserved=(0, 0, 0, 0), abi_version=ABI_VERSION):
        _lib()
        self.n_channels, self.corr_len = int(n_channels), int(corr_len)
        w = None if window is None else np.ascontiguousarray(window, np.int16)
        if w is not None and w.size != self.corr_len:
            raise ValueError("window must have corr_len entries")
        cfg = FskConfig(abi_version, self.n_channels, self.corr_len, int(mark_inc), int(space_inc), int(baud_inc), int(loop_shift), int(flags),
                        None if w is None else w.ctypes.data, int(min_len), int(max_len))
        for i in range(4):
            cfg.reserved[i] = int(reserved[i])
        self._create(engine, "fsk", C.byref(cfg))

    def max_frames(self, n):
        """iqd_fsk_max_frames: the records per channel a call of n samples needs"""
        return self._L.iqd_fsk_max_frames(self._h, int(n))

    def max_bit_words(self, n):
        """iqd_fsk_max_bit_words: the uint32 words per channel for the bits of a call of n samples"""
        return self._L.iqd_fsk_max_bit_words(self._h, int(n))

    def max_bytes(self, n):
        """iqd_fsk_max_bytes: the payload bytes per channel a call of n samples needs"""
        return self._L.iqd_fsk_max_bytes(self._h, int(n))

    def run(self, pcm, n=None, count=None, want_bits=True):
        """pcm [n_channels, row_stride] int16 (a host array), the first n samples of each row (count: [n_channels] uint32, fewer
        for some) -> (n_bits [n_channels] uint32, bits [n_channels, Bw] uint32 or None, n_frames [n_channels] uint32,
        frames [n_channels, F] FSK_FRAME, bytes [n_channels, Bc] uint8); synchronises."""
        pcm, stride, n, count = self._rows(pcm, n, count)
        F, Bw, Bc = self.max_frames(max(n, 0)), self.max_bit_words(max(n, 0)), self.max_bytes(max(n, 0))
        nb, nf = np.zeros(self.n_channels, np.uint32), np.zeros(self.n_channels, np.uint32)
        bits = np.zeros((self.n_channels, Bw), np.uint32) if want_bits else None
        frames = np.zeros((self.n_channels, F), FSK_FRAME)
        data = np.zeros((self.n_channels, Bc), np.uint8)
        self._e._check(self._L.iqd_fsk_run(self._e._h, self._h, capi._ptr_or_placeholder(pcm), stride, _np_ptr(count), n, _np_ptr(nb),
                                           None if bits is None else capi._ptr_or_placeholder(bits), _np_ptr(nf),
                                           capi._ptr_or_placeholder(frames), capi._ptr_or_placeholder(data)))
        return nb, bits, nf, frames, data

    def run_device(self, pcm_dev, row_stride, n, n_bits_dev, n_frames_dev, frames_dev, bytes_dev, bits_dev=0, count_dev=0, engine=None):
        """iqd_fsk_run_device: device pointers (integers), queued on the engine's stream."""
        self._run_device(engine, _dev_ptr(pcm_dev), int(row_stride), _dev_ptr(count_dev), int(n), _dev_ptr(n_bits_dev), _dev_ptr(bits_dev),
                         _dev_ptr(n_frames_dev), _dev_ptr(frames_dev), _dev_ptr(bytes_dev))


def frames_of(n_frames, frames, data):
    """[(channel, end_sample, payload bytes, fcs)] of a call's result, channel by channel in stream order"""
    return [(c, int(r["end_sample"]), data[c, int(r["offset"]):int(r["offset"]) + int(r["len"])].tobytes(), int(r["fcs"]))
            for c in range(len(n_frames)) for r in frames[c, :int(n_frames[c])]]
