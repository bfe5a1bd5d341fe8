"""The PCM tone bank of libiqdemod.so (include/iqdemod_tones.h: iqd_tones_*): which of T tones - CTCSS, DTMF, a 1750 Hz
burst - is in every channel's PCM, frame by frame, on the engine's stream.  An add-on: its functions have their own table
here, which capi._bind sets on the loaded library at first use; capi.PROTOTYPES is include/iqdemod.h alone."""
import ctypes as C

import numpy as np

from . import capi
from .capi import IqdError, _dev_ptr, _np_ptr, _ok

ABI_VERSION = 1
F_OPENED, F_CLOSED = 1, 2
NONE = 0xffffffff


class TonesConfig(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_channels", C.c_uint32), ("frame_len", C.c_uint32), ("n_tones", C.c_uint32),
                ("phase_inc", C.c_void_p), ("window", C.c_void_p), ("min_power", C.c_uint64), ("ratio_q8", C.c_uint32),
                ("energy_q8", C.c_uint32), ("open", C.c_uint32), ("hold", C.c_uint32), ("reserved", C.c_uint32 * 4)]


class TonesState(C.Structure):
    _fields_ = [("tone", C.c_int32), ("cand", C.c_int32), ("run", C.c_uint32), ("miss", C.c_uint32), ("fill", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


TONES_FRAME = np.dtype([("energy", "<u8"), ("p_best", "<u8"), ("p_second", "<u8"), ("best", "<u4"), ("second", "<u4"),
                        ("tone", "<i4"), ("flags", "<u4")])

_vp, _u32, _u64, _sz, _int, _P = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int, C.POINTER

# Every function of include/iqdemod_tones.h, in its order: name -> (what it returns, what it takes), as capi.PROTOTYPES.
# tests/test_tones_host.py holds this against the header.
PROTOTYPES = {
    "iqd_tones_create": (_int, (_vp, _P(TonesConfig), _P(_vp))),
    "iqd_tones_destroy": (None, (_vp,)),
    "iqd_tones_reset": (_int, (_vp,)),
    "iqd_tones_max_frames": (_sz, (_vp, _sz)),
    "iqd_tones_run_device": (_int, (_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp)),
    "iqd_tones_run": (_int, (_vp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _vp)),
    "iqd_tones_get_state": (_int, (_vp, _u32, _P(TonesState))),
    "iqd_tones_phase_inc": (_int, (_u64, _u32, _P(_u32))),
    "iqd_tones_default_window": (_int, (_u32, _vp)),
    "iqd_tones_ctcss": (_int, (_vp,)),
    "iqd_tones_dtmf": (_int, (_vp,)),
}


def _lib():
    """capi's library with this table's prototypes set (once)"""
    return capi._addon_lib(PROTOTYPES)


def phase_inc(freq_mhz, rate_hz):
    """iqd_tones_phase_inc (host only): a tone's phase increment from its frequency in millihertz and the PCM rate in Hz"""
    return capi._addon_phase_inc(PROTOTYPES, "tones", freq_mhz, rate_hz)


def default_window(frame_len):
    """iqd_tones_default_window (host only): the window used where none is given, [frame_len] int16"""
    w = np.zeros(max(int(frame_len), 0), np.int16)
    if not 0 <= int(frame_len) <= 0xffffffff or _lib().iqd_tones_default_window(int(frame_len), _np_ptr(w if w.size else np.zeros(1, np.int16))) != 0:
        raise IqdError(-1, "iqd_tones_default_window: frame_len %r must be a multiple of 32, 32 .. 8192" % (frame_len,))
    return w


def ctcss_mhz():
    """iqd_tones_ctcss: the 50 standard CTCSS tones in millihertz"""
    f = np.zeros(50, np.uint32)
    _ok(_lib().iqd_tones_ctcss(_np_ptr(f)), "iqd_tones_ctcss")
    return f


def dtmf_mhz():
    """iqd_tones_dtmf: the four row and four column frequencies of DTMF in millihertz"""
    f = np.zeros(8, np.uint32)
    _ok(_lib().iqd_tones_dtmf(_np_ptr(f)), "iqd_tones_dtmf")
    return f


CTCSS_DEFAULTS = dict(frame_len=4096, ratio_q8=512, open=2, hold=1, energy_q8=0, min_power=0)   # DESIGN 4.17 has the why


class Tones(capi._PcmChild):
    """iqd_tones_*: per channel and frame of frame_len PCM samples the power of each of the tones (phase_inc: one uint32 each),
    the best and the second, a hit by min_power, ratio_q8 and energy_q8, and a tone in force with hysteresis (open hits to
    open, more than hold misses to close).  Frames straddle calls; state is carried from call to call until reset().
    state(channel): dict(tone, cand, run, miss, fill)."""
    _State = TonesState

    def __init__(self, engine, n_channels, phase_inc, frame_len=4096, window=None, min_power=0, ratio_q8=512, energy_q8=0, open=2,
                 hold=1, reserved=(0, 0, 0, 0), abi_version=ABI_VERSION):
        _lib()
        inc = np.ascontiguousarray(phase_inc, np.uint32)
        self.n_channels, self.frame_len, self.n_tones = int(n_channels), int(frame_len), int(inc.size)
        w = None if window is None else np.ascontiguousarray(window, np.int16)
        if w is not None and w.size != self.frame_len:
            raise ValueError("window must have frame_len entries")
        cfg = TonesConfig(abi_version, self.n_channels, self.frame_len, self.n_tones, inc.ctypes.data if inc.size else None,
                          None if w is None else w.ctypes.data, int(min_power), int(ratio_q8), int(energy_q8), int(open), int(hold))
        for i in range(4):
            cfg.reserved[i] = int(reserved[i])
        self._create(engine, "tones", C.byref(cfg))

    def max_frames(self, n):
        """iqd_tones_max_frames: the frames a call of n samples can complete"""
        return self._L.iqd_tones_max_frames(self._h, int(n))

    def run(self, pcm, n=None, count=None, want_power=True):
        """pcm [n_channels, row_stride] int16 (a host array), the first n samples of each row (count: [n_channels] uint32, fewer
        for some) -> (n_frames [n_channels] uint32, frames [n_channels, F] TONES_FRAME, power [n_channels, F, n_tones] uint64 or
        None); synchronises."""
        pcm, stride, n, count = self._rows(pcm, n, count)
        F = self.max_frames(max(n, 0))
        nf = np.zeros(self.n_channels, np.uint32)
        frames = np.zeros((self.n_channels, F), TONES_FRAME)
        power = np.zeros((self.n_channels, F, self.n_tones), np.uint64) if want_power else None
        self._e._check(self._L.iqd_tones_run(self._e._h, self._h, capi._ptr_or_placeholder(pcm), stride, _np_ptr(count), n, _np_ptr(nf),
                                             capi._ptr_or_placeholder(frames), None if power is None else capi._ptr_or_placeholder(power)))
        return nf, frames, power

    def run_device(self, pcm_dev, row_stride, n, n_frames_dev, frames_dev, power_dev=0, count_dev=0, engine=None):
        """iqd_tones_run_device: device pointers (integers), queued on the engine's stream."""
        self._run_device(engine, _dev_ptr(pcm_dev), int(row_stride), _dev_ptr(count_dev), int(n), _dev_ptr(n_frames_dev), _dev_ptr(frames_dev),
                         _dev_ptr(power_dev))
