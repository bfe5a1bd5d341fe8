"""ctypes binding of include/iqdemod.h (libiqdemod.so).

Mirrors the C ABI one to one; the names, argument meaning and error behaviour are those of the
header, which in turn cites the reference's IqDataProcessor interface.  No torch types cross
this boundary: device buffers are passed as integer addresses.
"""
import ctypes as C
import os
import weakref

import numpy as np

from .build import LIB as _DEFAULT_LIB

LIB = os.environ.get("IQD_LIB", _DEFAULT_LIB)   # experiments: alternative builds of the same ABI

MODE = {"none": 0, "am": 1, "fm": 2, "wbfm": 3, "lsb": 4, "usb": 5}
DEMOD = {"am": 1, "fm": 2, "wbfm": 3, "ssb": 4}
F_NO_MAGNITUDE = 0x1
F_WBFM_TILES, F_WBFM_STREAM, F_PREPASS_OVERLAP = 0x2, 0x4, 0x8


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_channels", C.c_uint32), ("block_bytes", C.c_uint32),
                ("device", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class Stats(C.Structure):
    _fields_ = [("accepts", C.c_uint64), ("samples", C.c_uint64), ("kernel_launches", C.c_uint64),
                ("state_checks", C.c_uint64), ("state_repairs", C.c_uint64),
                ("chain_kernel_ms", C.c_double), ("chain_kernel_count", C.c_uint64), ("segment_repairs", C.c_uint64),
                ("stream_launches", C.c_uint64), ("device_launches", C.c_uint64), ("device_copies", C.c_uint64),
                ("mixed_launches", C.c_uint64)]


class AgcState(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("type", C.c_uint32), ("operating_point_dbfs", C.c_int32),
                ("deadband_db", C.c_uint32), ("blanking_limit", C.c_uint32), ("alpha", C.c_float),
                ("rx_gain_db", C.c_uint32), ("if_gain_db", C.c_uint32), ("filtered_if_gain_db", C.c_float),
                ("blanking_counter", C.c_uint32), ("gain_was_adjusted", C.c_uint32),
                ("normalized_level_dbfs", C.c_int32), ("signal_magnitude", C.c_uint32)]


class ChannelizerConfig(C.Structure):
    _fields_ = [("n_sources", C.c_uint32), ("n_channels", C.c_uint32), ("decimation", C.c_uint32),
                ("n_taps", C.c_uint32), ("taps", C.c_void_p), ("decimation_den", C.c_uint32),
                ("sample_format", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class SpectrumConfig(C.Structure):
    _fields_ = [("n_sources", C.c_uint32), ("n_bins", C.c_uint32), ("window", C.c_void_p),
                ("sample_format", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class DetectConfig(C.Structure):
    _fields_ = [("n_bins", C.c_uint32), ("floor_rank", C.c_uint32), ("ratio_q8", C.c_uint32), ("dc_guard", C.c_uint32),
                ("bridge", C.c_uint32), ("min_width", C.c_uint32), ("max_detections", C.c_uint32), ("reserved", C.c_uint32 * 1)]


class TrackConfig(C.Structure):
    _fields_ = [("n_sources", C.c_uint32), ("n_bins", C.c_uint32), ("max_detections", C.c_uint32), ("n_slots", C.c_uint32),
                ("gate_q8", C.c_uint32), ("open_hits", C.c_uint32), ("hold_blocks", C.c_uint32), ("alpha_q8", C.c_uint32),
                ("inc_bias", C.c_uint32), ("class_edge", C.c_uint32 * 3), ("reserved", C.c_uint32 * 4)]


# iqd_detect_row and iqd_detection (include/iqdemod.h: "Band activity") as numpy structured dtypes, 16 and 32 bytes
DETECT_ROW = np.dtype([("floor", "<u4"), ("threshold", "<u4"), ("n_found", "<u4"), ("n_hot_bins", "<u4")])
DETECTION = np.dtype([("first_bin", "<u4"), ("last_bin", "<u4"), ("peak_bin", "<u4"), ("peak_power", "<u4"),
                      ("sum_power", "<u8"), ("centroid_q8", "<u4"), ("n_hot", "<u4")])


# iqd_track_slot and iqd_track_block (include/iqdemod.h: "Band tracks"), 32 and 16 bytes
TRACK_SLOT = np.dtype([("track_id", "<u4"), ("state", "u1"), ("flags", "u1"), ("hits", "u1"), ("width_class", "u1"),
                       ("misses", "<u2"), ("max_width", "<u2"), ("centre_q8", "<u4"), ("phase_inc", "<u4"),
                       ("first_bin", "<u2"), ("last_bin", "<u2"), ("peak_power", "<u4"), ("age_blocks", "<u4")])
TRACK_BLOCK = np.dtype([("n_active", "<u4"), ("n_tentative", "<u4"), ("n_opened_closed", "<u4"), ("n_unplaced", "<u4")])


class MeasureConfig(C.Structure):
    """iqd_measure_config (include/iqdemod.h: "Band track measurements")"""
    _fields_ = [("n_sources", C.c_uint32), ("n_bins", C.c_uint32), ("n_slots", C.c_uint32), ("dc_guard", C.c_uint32),
                ("margin", C.c_uint32), ("obw_tail_q16", C.c_uint32), ("carrier_half", C.c_uint32), ("min_sum", C.c_uint32),
                ("carrier_min_q8", C.c_uint32), ("wide_bins", C.c_uint32), ("reserved", C.c_uint32 * 2)]


# iqd_track_measure (include/iqdemod.h: "Band track measurements"), 32 bytes
TRACK_MEASURE = np.dtype([("track_id", "<u4"), ("obw_lo", "<u2"), ("obw_hi", "<u2"), ("peak_bin", "<u2"), ("flags", "u1"),
                          ("hint", "u1"), ("peak_excess", "<u4"), ("centroid_q8", "<u4"), ("carrier_q8", "<u2"),
                          ("n_over", "<u2"), ("sum_excess", "<u8")])
MEASURE_F_EMPTY, MEASURE_F_WEAK = 1, 2
HINT_NONE, HINT_CARRIER, HINT_NARROW, HINT_WIDE = 0, 1, 2, 3
HINT_MODE = {HINT_NONE: "fm", HINT_CARRIER: "am", HINT_NARROW: "fm", HINT_WIDE: "wbfm"}   # what iqdemod_wide modes=auto sets


class TrackLogConfig(C.Structure):
    """iqd_tracklog_config (include/iqdemod.h: "Band track log")"""
    _fields_ = [("n_sources", C.c_uint32), ("n_slots", C.c_uint32), ("max_events", C.c_uint32), ("min_active", C.c_uint32),
                ("vote_min", C.c_uint32), ("reserved", C.c_uint32 * 3)]


# iqd_track_summary and iqd_tracklog_counts (include/iqdemod.h: "Band track log"), 64 and 16 bytes
TRACK_SUMMARY = np.dtype([("track_id", "<u4"), ("state", "u1"), ("flags", "u1"), ("mode_hint", "u1"), ("width_class", "u1"),
                          ("first_block", "<u8"), ("n_blocks", "<u4"), ("n_active", "<u4"), ("n_measured", "<u4"),
                          ("votes", "<u4", (3,)), ("sum_centre_q8", "<u8"), ("sum_excess", "<u8"), ("peak_excess", "<u4"),
                          ("obw_lo_min", "<u2"), ("obw_hi_max", "<u2")])
TRACKLOG_COUNTS = np.dtype([("n_events", "<u4"), ("n_stored", "<u4"), ("n_short", "<u4"), ("n_lost", "<u4")])
TLOG_F_NEW, TLOG_F_MODE_CHANGED, TLOG_F_CLOSED, TLOG_F_LOST = 1, 2, 4, 8


class TrackFollow(C.Structure):
    """iqd_track_follow (include/iqdemod.h: "Track-following channels")"""
    _fields_ = [("slots_dev", C.c_void_p), ("n_slots", C.c_uint32), ("n_blocks", C.c_uint32), ("block_bytes", C.c_uint32),
                ("lag", C.c_uint32), ("min_state", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class IqdError(RuntimeError):
    def __init__(self, status, detail):
        super().__init__("libiqdemod: %s (%d): %s" % (_lib().iqd_strerror(status).decode(), status, detail))
        self.status = status


_vp, _u32, _u64, _sz, _int, _P = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int, C.POINTER

# Every function of include/iqdemod.h, in its order: name -> (what it returns, what it takes).  Handles, device and host
# buffers are c_void_p; POINTER(...) is where callers pass byref().  tests/test_abi_prototypes.py holds this against the header.
PROTOTYPES = {
    "iqd_create": (_int, (_P(Config), _P(_vp))),
    "iqd_destroy": (None, (_vp,)),
    "iqd_set_mode": (_int, (_vp, _u32, _u32, _int)),
    "iqd_set_gain": (_int, (_vp, _u32, _u32, _int, C.c_float)),
    "iqd_set_squelch": (_int, (_vp, _u32, _u32, C.c_int32)),
    "iqd_set_rx_gain_db": (_int, (_vp, _u32, _u32, _u32)),
    "iqd_get_rx_gain_db": (_int, (_vp, _u32, _P(_u32))),
    "iqd_agc_set_type": (_int, (_vp, _u32, _u32, _u32)),
    "iqd_agc_set_deadband": (_int, (_vp, _u32, _u32, _u32)),
    "iqd_agc_set_blanking_limit": (_int, (_vp, _u32, _u32, _u32)),
    "iqd_agc_set_operating_point": (_int, (_vp, _u32, _u32, C.c_int32)),
    "iqd_agc_set_filter_coefficient": (_int, (_vp, _u32, _u32, C.c_float)),
    "iqd_agc_enable": (_int, (_vp, _u32, _u32, _int)),
    "iqd_agc_get_state": (_int, (_vp, _u32, _P(AgcState))),
    "iqd_scanner_set_parameters": (_int, (_vp, _u32, _u32, _u64, _u64, _u64)),
    "iqd_scanner_start": (_int, (_vp, _u32, _u32, _int)),
    "iqd_scanner_get": (_int, (_vp, _u32, _P(_u64), _P(_u64), _P(_int))),
    "iqd_set_gain_trace": (_int, (_vp, _int)),
    "iqd_get_gain_trace": (_int, (_vp, _u32, _u32, _vp, _sz)),
    "iqd_get_frequency_trace": (_int, (_vp, _u32, _u32, _vp, _sz)),
    "iqd_set_rotation": (_int, (_vp, _u32, _u32, _int)),
    "iqd_reset": (_int, (_vp, _u32, _u32)),
    "iqd_reset_demod": (_int, (_vp, _u32, _u32, _int)),
    "iqd_accept_iq": (_int, (_vp, _u32, _u32, _vp, _sz, _vp, _vp, _vp, _vp)),
    "iqd_accept_iq_device": (_int, (_vp, _u32, _u32, _vp, _sz, _vp, _vp, _vp, _vp)),
    "iqd_synchronize": (_int, (_vp,)),
    "iqd_demod_accept": (_int, (_vp, _u32, _u32, _int, _vp, _sz, _vp)),
    "iqd_demod_set_sideband": (_int, (_vp, _u32, _u32, _int)),
    "iqd_front_end": (_int, (_vp, _u32, _u32, _vp, _sz, _vp)),
    "iqd_front_end_device": (_int, (_vp, _u32, _u32, _vp, _sz, _vp)),
    "iqd_convert_fs_over_4": (_int, (_vp, _int, _vp, _sz)),
    "iqd_get_stats": (_int, (_vp, _P(Stats))),
    "iqd_set_profiling": (_int, (_vp, _int)),
    "iqd_get_channel_mode": (_int, (_vp, _u32, _P(_int))),
    "iqd_get_channel_gain": (_int, (_vp, _u32, _int, _P(C.c_float))),
    "iqd_last_error": (C.c_char_p, (_vp,)),
    "iqd_strerror": (C.c_char_p, (_int,)),
    "iqd_abi_version": (_u32, ()),
    "iqd_resampler_create": (_int, (_vp, _int, _vp, _u32, _u32, _u32, _P(_vp))),
    "iqd_resampler_destroy": (None, (_vp,)),
    "iqd_resampler_reset": (_int, (_vp,)),
    "iqd_resampler_out_count": (_sz, (_vp, _sz)),
    "iqd_resampler_run": (_int, (_vp, _vp, _sz, _vp)),
    "iqd_resampler_run_device": (_int, (_vp, _vp, _sz, _vp)),
    "iqd_filter_create": (_int, (_vp, _int, _vp, _u32, _vp, _u32, _u32, _u32, _P(_vp))),
    "iqd_filter_destroy": (None, (_vp,)),
    "iqd_filter_reset": (_int, (_vp,)),
    "iqd_filter_out_count": (_sz, (_vp, _sz)),
    "iqd_filter_run": (_int, (_vp, _vp, _sz, _vp)),
    "iqd_filter_run_device": (_int, (_vp, _vp, _sz, _vp)),
    "iqd_filter_tile_samples": (_u32, (_int, _u32, _u32, _u32)),
    "iqd_filter_clamp_free_taps": (_u32, (_vp, _u32)),
    "iqd_channelizer_create": (_int, (_vp, _P(ChannelizerConfig), _P(_vp))),
    "iqd_channelizer_destroy": (None, (_vp,)),
    "iqd_channelizer_reset": (_int, (_vp,)),
    "iqd_channelizer_set_channels": (_int, (_vp, _u32, _u32, _vp, _vp, _vp)),
    "iqd_channelizer_run_device": (_int, (_vp, _vp, _sz, _vp)),
    "iqd_channelizer_run": (_int, (_vp, _vp, _sz, _vp)),
    "iqd_accept_wideband": (_int, (_vp, _vp, _u32, _vp, _sz, _vp, _vp, _vp, _vp)),
    "iqd_channelizer_phasor_table": (_int, (_vp,)),
    "iqd_channelizer_default_taps": (_int, (_u32, _vp, _u32)),
    "iqd_channelizer_default_taps_q": (_int, (_u32, _u32, _vp, _u32)),
    "iqd_channelizer_window_outputs": (_u32, (_u32, _u32, _u32)),
    "iqd_channelizer_set_source_frequency": (_int, (_vp, _u32, _u32, _vp)),
    "iqd_channelizer_follow_scanner": (_int, (_vp, _u32, _u32, _int)),
    "iqd_channelizer_tuning": (_int, (_u32, _u64, _u64, _int, _P(_u32))),
    "iqd_accept_wideband_device": (_int, (_vp, _vp, _u32, _vp, _sz, _vp, _vp, _vp, _vp, _vp)),
    "iqd_channelizer_follow_gain": (_int, (_vp, _u32, _u32, _int)),
    "iqd_channelizer_set_survey": (_int, (_vp, _u32, _vp, _vp)),
    "iqd_channelizer_survey_device": (_int, (_vp, _vp, _sz, _u32, _vp)),
    "iqd_channelizer_survey": (_int, (_vp, _vp, _sz, _u32, _vp)),
    "iqd_magnitude_dbfs": (C.c_int32, (_u32,)),
    "iqd_spectrum_create": (_int, (_vp, _P(SpectrumConfig), _P(_vp))),
    "iqd_spectrum_destroy": (None, (_vp,)),
    "iqd_spectrum_run_device": (_int, (_vp, _vp, _sz, _u32, _vp)),
    "iqd_spectrum_run": (_int, (_vp, _vp, _sz, _u32, _vp)),
    "iqd_spectrum_default_window": (_int, (_u32, _vp)),
    "iqd_spectrum_full_scale": (_int, (_vp, _u32, _P(_u32))),
    "iqd_detect_create": (_int, (_vp, _P(DetectConfig), _P(_vp))),
    "iqd_detect_destroy": (None, (_vp,)),
    "iqd_detect_run_device": (_int, (_vp, _vp, _sz, _vp, _vp)),
    "iqd_detect_run": (_int, (_vp, _vp, _sz, _vp, _vp)),
    "iqd_detect_offset_hz": (_int, (_u32, _u32, _u32, _P(C.c_int64))),
    "iqd_track_create": (_int, (_vp, _P(TrackConfig), _P(_vp))),
    "iqd_track_destroy": (None, (_vp,)),
    "iqd_track_reset": (_int, (_vp,)),
    "iqd_track_run_device": (_int, (_vp, _vp, _vp, _sz, _vp, _vp)),
    "iqd_track_run": (_int, (_vp, _vp, _vp, _sz, _vp, _vp)),
    "iqd_track_get_state": (_int, (_vp, _u32, _vp)),
    "iqd_track_phase_inc": (_int, (_u32, _u32, _u32, _P(_u32))),
    "iqd_channelizer_set_track_table": (_int, (_vp, _P(TrackFollow))),
    "iqd_channelizer_follow_tracks": (_int, (_vp, _u32, _u32, _vp)),
    "iqd_channelizer_track_window_outputs": (_u32, (_u32, _u32)),
    "iqd_measure_create": (_int, (_vp, _P(MeasureConfig), _P(_vp))),
    "iqd_measure_destroy": (None, (_vp,)),
    "iqd_measure_run_device": (_int, (_vp, _vp, _vp, _vp, _sz, _vp)),
    "iqd_measure_run": (_int, (_vp, _vp, _vp, _vp, _sz, _vp)),
    "iqd_tracklog_create": (_int, (_vp, _P(TrackLogConfig), _P(_vp))),
    "iqd_tracklog_destroy": (None, (_vp,)),
    "iqd_tracklog_reset": (_int, (_vp,)),
    "iqd_tracklog_run_device": (_int, (_vp, _vp, _vp, _sz, _vp, _vp, _vp)),
    "iqd_tracklog_run": (_int, (_vp, _vp, _vp, _sz, _vp, _vp, _vp)),
    "iqd_tracklog_get_state": (_int, (_vp, _u32, _vp, _P(_u64))),
    "iqd_tracklog_mean_centre": (_int, (_u64, _u32, _P(_u32))),
    "iqd_gather_unique_id": (_int, (_vp,)),
    "iqd_gather_create": (_int, (_vp, C.c_char_p, _u32, _u32, _u32, _P(_vp))),
    "iqd_gather_pcm": (_int, (_vp, _vp, _P(_sz), _vp, _sz)),
    "iqd_gather_destroy": (None, (_vp,)),
    "iqd_gather_info": (_int, (_vp, _P(_int), _P(_int), _P(_int))),
    "iqd_dev_alloc": (_int, (_vp, _sz, _P(_vp))),
    "iqd_dev_free": (_int, (_vp, _vp)),
    "iqd_dev_upload": (_int, (_vp, _vp, _vp, _sz)),
    "iqd_dev_download": (_int, (_vp, _vp, _vp, _sz)),
    "iqd_host_alloc": (_int, (_vp, _sz, _P(_vp))),
    "iqd_host_free": (_int, (_vp, _vp)),
    "iqd_dev_tile": (_int, (_vp, _vp, _sz, _sz)),
    "iqd_stream": (_vp, (_vp,)),
    "iqd_device_count": (_int, ()),
    "iqd_get_device": (_int, (_vp, _P(_int))),
    "iqd_debug_stamps": (_int, (_vp, _vp)),
    "iqd_debug_stamps_ext": (_int, (_vp, _vp, _u32)),
}
EXPORTS = list(PROTOTYPES)

_LIB = None


def _bind(L, table=None):
    """Gives every function of `L` its prototype (a library without one of them raises); returns L.  `table`: an add-on's
    table (tones.PROTOTYPES) instead of this module's."""
    for name, (restype, argtypes) in (PROTOTYPES if table is None else table).items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, list(argtypes)
    return L


def _lib():
    """Loads libiqdemod.so (raises if it has not been built — there is no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB):
            raise FileNotFoundError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB)
        _LIB = _bind(C.CDLL(LIB))
    return _LIB


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _dev_ptr(x):
    """a device pointer argument: an integer address; 0 or None is NULL"""
    return C.c_void_p(x or None)


def _ptr_or_placeholder(a):
    """_np_ptr(a), but an empty array - its call is refused or writes nothing - gets a valid pointer all the same"""
    return _np_ptr(a if a.size else np.zeros(64, np.uint8))


def _ok(rc, detail):
    """for calls that leave no text with an engine: a status other than IQD_OK raises with `detail`"""
    if rc != 0:
        raise IqdError(rc, detail)


def _u32_config(cls, values, **arrays):
    """cls(*values), its array fields filled entry by entry from `arrays`, every value taken modulo 2^32"""
    cfg = cls(*[int(v) & 0xffffffff for v in values])
    for name, vals in arrays.items():
        field = getattr(cfg, name)
        for i in range(len(field)):
            field[i] = int(vals[i]) & 0xffffffff
    return cfg


def _u32_function(name, out, args, detail, bits=32):
    """A host-only function of unsigned arguments (the first of `bits` bits, the others of 32) that fills `out`: an argument
    out of range, like any refusal of the library's, is IQD_EINVAL with `detail`."""
    args = [int(v) for v in args]
    if not all(0 <= v < 2 ** b for v, b in zip(args, [bits, 32, 32])) or getattr(_lib(), name)(*args, C.byref(out)) != 0:
        raise IqdError(-1, detail)
    return out.value


class _EngineChild:
    """An object that queues on its engine's stream: made by iqd_<kind>_create, registered so that Engine.close() closes it
    first, gone by iqd_<kind>_destroy.  _h is what the raw library takes."""
    _e = _L = _h = _kind = None

    def _create(self, engine, kind, *args, failed=None):
        """iqd_<kind>_create(engine, *args, &handle); `failed` is the error's text where the engine keeps none"""
        self._e, self._L, self._kind = engine, engine._L, kind
        h = C.c_void_p()
        rc = getattr(self._L, "iqd_%s_create" % kind)(engine._h, *args, C.byref(h))
        if failed:
            _ok(rc, failed)
        engine._check(rc)
        self._h = h
        engine._children.add(self)

    def close(self):
        """iqd_<kind>_destroy; Engine.close() calls it first, so it never runs on a destroyed engine's stream."""
        if self._h and self._e._h:
            getattr(self._L, "iqd_%s_destroy" % self._kind)(self._h)
        self._h = None

    __del__ = close


# ---- PCM add-ons (tones.py, fsk.py): an add-on's functions have their own table in its module; this module's is iqdemod.h alone
_ADDONS_BOUND = set()


def _addon_lib(prototypes):
    """_lib() with an add-on's PROTOTYPES set on it (once per table)"""
    if id(prototypes) not in _ADDONS_BOUND:
        _bind(_lib(), prototypes)
        _ADDONS_BOUND.add(id(prototypes))
    return _lib()


def _addon_phase_inc(prototypes, kind, freq_mhz, rate_hz):
    """iqd_<kind>_phase_inc (host only): a phase increment from a frequency in millihertz and the PCM rate in Hz"""
    _addon_lib(prototypes)
    return _u32_function("iqd_%s_phase_inc" % kind, C.c_uint32(), (freq_mhz, rate_hz),
                         "iqd_%s_phase_inc: freq_mhz %r must be below 500 rate_hz (%r), rate_hz not 0" % (kind, freq_mhz, rate_hz), bits=64)


class _PcmChild(_EngineChild):
    """An add-on on [n_channels, row_stride] int16 rows with state per channel.  A subclass names _State, the ctypes mirror of
    its get_state record, and sets n_channels before _create."""
    _State = None

    def _fn(self, name):
        return getattr(self._L, "iqd_%s_%s" % (self._kind, name))

    def _rows(self, pcm, n, count):
        """run's first arguments as the library takes them: (pcm [n_channels, row_stride] int16, row_stride, n, count or None)"""
        pcm = np.ascontiguousarray(pcm, np.int16).reshape(self.n_channels, -1)
        stride = pcm.shape[1]
        return pcm, stride, stride if n is None else int(n), None if count is None else np.ascontiguousarray(count, np.uint32)

    def _run_device(self, engine, *args):
        """iqd_<kind>_run_device on `engine` or the object's own; a refusal's text is the object's engine's"""
        self._e._check(self._fn("run_device")((self._e if engine is None else engine)._h, self._h, *args))

    def reset(self):
        """iqd_<kind>_reset: every channel's carried state cleared."""
        self._e._check(self._fn("reset")(self._h))

    def state(self, channel=0):
        """iqd_<kind>_get_state: one channel's record as a dict of integers (without `reserved`); synchronises."""
        s = self._State()
        if not 0 <= int(channel) <= 0xffffffff:
            raise IqdError(-1, "iqd_%s_get_state: channel %r out of range" % (self._kind, channel))
        self._e._check(self._fn("get_state")(self._h, int(channel), C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in self._State._fields_ if k != "reserved"}


class Engine:
    """N independent channels, each one reference IqDataProcessor + its four demodulators."""

    def __init__(self, n_channels=1, block_bytes=0, device=-1, flags=0):
        self._h, self._children, self._pinned = C.c_void_p(), weakref.WeakSet(), {}    # (what close() needs, first)
        self._L = _lib()
        cfg = Config(self._L.iqd_abi_version(), n_channels, block_bytes, device, flags)
        rc = self._L.iqd_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise IqdError(rc, "iqd_create failed (is a HIP device visible?)")
        self.n_channels = n_channels
        self.block_bytes = block_bytes or 32768

    def close(self):
        for child in list(self._children):   # every _EngineChild goes before its engine (include/iqdemod.h)
            child.close()
        if self._h:
            self._L.iqd_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise IqdError(rc, self._L.iqd_last_error(self._h).decode())

    def _range(self, first, n):
        return first, (self.n_channels - first if n is None else n)

    def _unless_refused(self, rc, refusals=(-6,)):
        """True / False like the reference's setters: IQD_EALREADY (for the AGC's, IQD_EINVAL too) is their `false`"""
        if rc in refusals:
            return False
        self._check(rc)
        return True

    # ---- the reference's control surface -------------------------------------------------
    def set_mode(self, mode, first=0, n=None):
        f, n = self._range(first, n)
        self._check(self._L.iqd_set_mode(self._h, f, n, int(MODE.get(mode, mode))))

    def set_gain(self, demod, gain, first=0, n=None):
        f, n = self._range(first, n)
        self._check(self._L.iqd_set_gain(self._h, f, n, int(DEMOD.get(demod, demod)), C.c_float(gain)))

    def set_squelch(self, threshold, first=0, n=None):
        f, n = self._range(first, n)
        self._check(self._L.iqd_set_squelch(self._h, f, n, int(threshold)))

    def set_rx_gain_db(self, gain_db, first=0, n=None):
        f, n = self._range(first, n)
        self._check(self._L.iqd_set_rx_gain_db(self._h, f, n, int(gain_db)))

    def set_rotation(self, rotation, first=0, n=None):
        f, n = self._range(first, n)
        self._check(self._L.iqd_set_rotation(self._h, f, n, int(rotation)))

    def reset(self, first=0, n=None):
        f, n = self._range(first, n)
        self._check(self._L.iqd_reset(self._h, f, n))

    def reset_demod(self, demod, first=0, n=None):
        f, n = self._range(first, n)
        self._check(self._L.iqd_reset_demod(self._h, f, n, int(DEMOD.get(demod, demod))))

    def demod_accept(self, demod, iq_s8, first=0, n=None):
        """{Am,Fm,WbFm,Ssb}Demodulator::acceptIqData: SIGNED bytes [n][bytes] (or one row) straight into the
        demodulator, no squelch; 'lsb' / 'usb' select the sideband first, like the reference's harness does."""
        f, n = self._range(first, n)
        if demod in ("lsb", "usb"):
            self._check(self._L.iqd_demod_set_sideband(self._h, f, n, 1 if demod == "lsb" else 0))
            demod = "ssb"
        iq_s8 = np.ascontiguousarray(iq_s8, dtype=np.int8)
        one = iq_s8.ndim == 1
        rows = iq_s8.reshape(n, -1)
        pcm = np.zeros((n, rows.shape[1] // 64), np.int16)
        self._check(self._L.iqd_demod_accept(self._h, f, n, int(DEMOD.get(demod, demod)), _np_ptr(rows), rows.shape[1], _np_ptr(pcm)))
        return pcm[0] if one else pcm

    # ---- AutomaticGainControl: True/False like the reference's setters -----------------------
    def _agc(self, fn, value, first, n):
        f, n = self._range(first, n)
        return self._unless_refused(fn(self._h, f, n, value), (-1, -6))

    def agc_set_type(self, t, first=0, n=None):
        return self._agc(self._L.iqd_agc_set_type, int(t), first, n)

    def agc_set_deadband(self, db, first=0, n=None):
        return self._agc(self._L.iqd_agc_set_deadband, int(db), first, n)

    def agc_set_blanking_limit(self, limit, first=0, n=None):
        return self._agc(self._L.iqd_agc_set_blanking_limit, int(limit), first, n)

    def agc_set_operating_point(self, dbfs, first=0, n=None):
        return self._agc(self._L.iqd_agc_set_operating_point, int(dbfs), first, n)

    def agc_set_filter_coefficient(self, a, first=0, n=None):
        return self._agc(self._L.iqd_agc_set_filter_coefficient, C.c_float(a), first, n)

    def agc_enable(self, on=True, first=0, n=None):
        return self._agc(self._L.iqd_agc_enable, 1 if on else 0, first, n)

    def agc_state(self, ch):
        st = AgcState()
        self._check(self._L.iqd_agc_get_state(self._h, ch, C.byref(st)))
        return {k: getattr(st, k) for k, _ in AgcState._fields_}

    def rx_gain_db(self, ch=0):
        g = C.c_uint32()
        self._check(self._L.iqd_get_rx_gain_db(self._h, ch, C.byref(g)))
        return g.value

    def set_gain_trace(self, on=True):
        self._check(self._L.iqd_set_gain_trace(self._h, 1 if on else 0))

    def gain_trace(self, n_blocks, first=0, n=None):
        f, n = self._range(first, n)
        out = np.zeros((n, n_blocks), np.uint32)
        self._check(self._L.iqd_get_gain_trace(self._h, f, n, _np_ptr(out), n_blocks))
        return out

    # ---- FrequencyScanner -------------------------------------------------------------------
    def scanner_set_parameters(self, start_hz, end_hz, increment_hz, first=0, n=None):
        f, n = self._range(first, n)
        return self._unless_refused(self._L.iqd_scanner_set_parameters(self._h, f, n, int(start_hz), int(end_hz), int(increment_hz)))

    def scanner_start(self, start=True, first=0, n=None):
        f, n = self._range(first, n)
        return self._unless_refused(self._L.iqd_scanner_start(self._h, f, n, 1 if start else 0))

    def scanner_tuned(self, ch=0):
        """(frequency the radio was last told to tune to, number of tuning commands)"""
        hz, n, sc = C.c_uint64(), C.c_uint64(), C.c_int()
        self._check(self._L.iqd_scanner_get(self._h, ch, C.byref(hz), C.byref(n), C.byref(sc)))
        return hz.value, n.value

    def frequency_trace(self, n_blocks, first=0, n=None):
        f, n = self._range(first, n)
        out = np.zeros((n, n_blocks), np.uint64)
        self._check(self._L.iqd_get_frequency_trace(self._h, f, n, _np_ptr(out), n_blocks))
        return out

    # ---- data path ------------------------------------------------------------------------
    def accept(self, iq_u8, first=0, n=None):
        """iq_u8: [n_ch, bytes_per_ch] uint8 host array.  Returns (pcm rows, counts, magnitude, allowed)."""
        f, n = self._range(first, n)
        iq_u8 = np.ascontiguousarray(iq_u8, dtype=np.uint8).reshape(n, -1)
        bpc = iq_u8.shape[1]
        nblk = bpc // self.block_bytes if bpc % self.block_bytes == 0 else 0
        pcm = np.zeros((n, bpc // 64), dtype=np.int16)
        cnt = np.zeros(n, dtype=np.uint32)
        mag = np.zeros((n, max(nblk, 1)), dtype=np.uint32)
        allowed = np.zeros((n, max(nblk, 1)), dtype=np.uint8)
        self._check(self._L.iqd_accept_iq(self._h, f, n, _np_ptr(iq_u8), bpc, _np_ptr(pcm), _np_ptr(cnt),
                                          _np_ptr(mag), _np_ptr(allowed)))
        return pcm, cnt, mag, allowed

    def accept_wideband(self, chz, wide_u8, first=0):
        """iqd_accept_wideband: one call's [n_sources, bytes_per_source] uint8 capture through the channelizer `chz` into
        engine channels [first, first + chz.n_channels).  Returns (pcm rows, counts, magnitude, allowed) like accept().
        A channelizer of sample_format "s8" / "s16" takes [n_sources, 2 samples] int8 / int16 (else TypeError)."""
        wide = chz._capture(wide_u8)
        bps = wide.shape[1]
        row, n = bps // (chz.decimation * chz.rail_bytes) * chz.decimation_den, chz.n_channels
        nblk = row // self.block_bytes if row % self.block_bytes == 0 else 1
        pcm = np.zeros((n, row // 64), dtype=np.int16)
        cnt = np.zeros(n, dtype=np.uint32)
        mag = np.zeros((n, nblk), dtype=np.uint32)
        allowed = np.zeros((n, nblk), dtype=np.uint8)
        self._check(self._L.iqd_accept_wideband(self._h, chz._h, first, _np_ptr(wide), bps, _np_ptr(pcm), _np_ptr(cnt),
                                                _np_ptr(mag), _np_ptr(allowed)))
        return pcm, cnt, mag, allowed

    def accept_wideband_device(self, chz, wide_dev, bytes_per_source, rows_dev, pcm_dev, count_dev=0, mag_dev=0,
                               allowed_dev=0, first=0):
        """iqd_accept_wideband_device: device pointers (integers), queued on the engine's stream; rows_dev receives the
        cut rows [n_channels, bytes_per_source / M] (fractional: bytes_per_source Q / P)."""
        self._check(self._L.iqd_accept_wideband_device(self._h, chz._h, int(first), C.c_void_p(wide_dev), int(bytes_per_source),
                                                       C.c_void_p(rows_dev), C.c_void_p(pcm_dev), _dev_ptr(count_dev),
                                                       _dev_ptr(mag_dev), _dev_ptr(allowed_dev)))

    def front_end(self, iq_u8, first=0, n=None):
        """u8 -> s8 -> rotation only: the bytes the reference leaves in its buffer / dumps over UDP."""
        f, n = self._range(first, n)
        iq_u8 = np.ascontiguousarray(iq_u8, dtype=np.uint8).reshape(n, -1)
        out = np.zeros(iq_u8.shape, np.int8)
        self._check(self._L.iqd_front_end(self._h, f, n, _np_ptr(iq_u8), iq_u8.shape[1], _np_ptr(out)))
        return out

    def convert_fs_over_4(self, direction, s8):
        """IqDataProcessor::upconvertByFsOver4 (+1) / downconvertByFsOver4 (-1) on a copy of signed bytes."""
        buf = np.array(s8, dtype=np.int8, copy=True)
        self._check(self._L.iqd_convert_fs_over_4(self._h, int(direction), _np_ptr(buf), buf.size))
        return buf

    def accept_device(self, iq_dev, bytes_per_ch, pcm_dev, count_dev=0, mag_dev=0, allowed_dev=0, first=0, n=None):
        f, n = self._range(first, n)
        self._check(self._L.iqd_accept_iq_device(self._h, f, n, C.c_void_p(iq_dev), bytes_per_ch,
                                                 C.c_void_p(pcm_dev), _dev_ptr(count_dev),
                                                 _dev_ptr(mag_dev), _dev_ptr(allowed_dev)))

    def synchronize(self):
        self._check(self._L.iqd_synchronize(self._h))

    def stream_handle(self):
        """The hipStream_t the engine launches on (an integer, for torch.cuda.ExternalStream)."""
        return int(self._L.iqd_stream(self._h) or 0)

    # ---- diagnostics / device helpers -------------------------------------------------------
    def stats(self):
        s = Stats()
        self._check(self._L.iqd_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def set_profiling(self, on):
        self._check(self._L.iqd_set_profiling(self._h, 1 if on else 0))

    def channel_mode(self, ch):
        m = C.c_int()
        self._check(self._L.iqd_get_channel_mode(self._h, ch, C.byref(m)))
        return m.value

    def channel_gain(self, ch, demod):
        g = C.c_float()
        self._check(self._L.iqd_get_channel_gain(self._h, ch, int(DEMOD.get(demod, demod)), C.byref(g)))
        return g.value

    def debug_stamps_ext(self, n=64):
        out = (C.c_ulonglong * n)()
        self._check(self._L.iqd_debug_stamps_ext(self._h, out, n))
        return list(out)

    def debug_stamps(self):
        out = (C.c_ulonglong * 16)()
        self._check(self._L.iqd_debug_stamps(self._h, out))
        return list(out)

    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._check(self._L.iqd_dev_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, ptr):
        self._check(self._L.iqd_dev_free(self._h, C.c_void_p(ptr)))

    def dev_upload(self, dst, host_array):
        a = np.ascontiguousarray(host_array)
        self._check(self._L.iqd_dev_upload(self._h, C.c_void_p(dst), _np_ptr(a), a.nbytes))

    def dev_download(self, src, nbytes, dtype=np.uint8):
        out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        self._check(self._L.iqd_dev_download(self._h, _np_ptr(out), C.c_void_p(src), nbytes))
        return out

    def host_array(self, shape, dtype=np.uint8):
        """A page-locked numpy array (iqd_host_alloc); free it with host_free(array)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._check(self._L.iqd_host_alloc(self._h, n, C.byref(p)))
        buf = (C.c_uint8 * n).from_address(p.value)
        a = np.frombuffer(buf, dtype=dtype).reshape(shape)
        self._pinned[a.ctypes.data] = p.value
        return a

    def host_free(self, a):
        p = self._pinned.pop(a.ctypes.data, None)
        if p is not None:
            self._check(self._L.iqd_host_free(self._h, C.c_void_p(p)))

    def accept_into(self, iq_u8, pcm, cnt=None, mag=None, allowed=None, first=0, n=None):
        """iqd_accept_iq on caller-owned host arrays (e.g. page-locked ones from host_array)."""
        f, n = self._range(first, n)
        bpc = iq_u8.size // n
        self._check(self._L.iqd_accept_iq(self._h, f, n, _np_ptr(iq_u8), bpc, _np_ptr(pcm), _np_ptr(cnt),
                                          _np_ptr(mag), _np_ptr(allowed)))

    def dev_tile(self, dst, period, total):
        self._check(self._L.iqd_dev_tile(self._h, C.c_void_p(dst), period, total))


class Gatherer(_EngineChild):
    """iqd_gather_*: this rank's PCM to row `rank` of a buffer on the root, over RCCL, on the engine's stream."""

    def __init__(self, engine, unique_id, rank, world, root=0):
        self.rank, self.world, self.root = rank, world, root
        self._create(engine, "gather", bytes(unique_id), rank, world, root, failed="iqd_gather_create failed (is librccl.so there?)")

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        _ok(_lib().iqd_gather_unique_id(buf), "iqd_gather_unique_id failed (is librccl.so there?)")
        return bytes(buf)

    def gather(self, send_dev, bytes_per_rank, recv_dev, row_stride):
        arr = (C.c_size_t * self.world)(*[int(b) for b in bytes_per_rank])
        _ok(self._L.iqd_gather_pcm(self._h, C.c_void_p(send_dev), arr, _dev_ptr(recv_dev), int(row_stride)), "iqd_gather_pcm failed")

    def info(self):
        """{'version': RCCL's version code, 'ranks': what ncclCommCount says, 'library_reused': the process's own copy}"""
        v, n, r = C.c_int(), C.c_int(), C.c_int()
        _ok(self._L.iqd_gather_info(self._h, C.byref(v), C.byref(n), C.byref(r)), "iqd_gather_info failed")
        return {"version": v.value, "ranks": n.value, "library_reused": bool(r.value)}


class Resampler(_EngineChild):
    """Block-wise Decimator / Interpolator / Interpolator_int16 for n_channels streams (include/iqdemod.h)."""
    KINDS = {"decimate_f32": 0, "interpolate_f32": 1, "interpolate_i16": 2}

    def __init__(self, engine, kind, taps, factor, n_channels=1):
        self.kind, self.n_ch = self.KINDS[kind], n_channels
        taps = np.ascontiguousarray(taps, np.float32)
        self._create(engine, "resampler", self.kind, _np_ptr(taps), len(taps), int(factor), n_channels)
        self.dtype = np.int16 if self.kind == 2 else np.float32

    def run(self, x):
        x = np.ascontiguousarray(x, self.dtype).reshape(self.n_ch, -1)
        out = np.zeros((self.n_ch, self._L.iqd_resampler_out_count(self._h, x.shape[1])), self.dtype)
        self._e._check(self._L.iqd_resampler_run(self._h, _np_ptr(x), x.shape[1], _np_ptr(out)))
        return out

    def reset(self):
        self._e._check(self._L.iqd_resampler_reset(self._h))


class Filter(_EngineChild):
    """Block-wise Decimator_int16 / FirFilter_int16 / FirFilter / IirFilter for n_channels streams (include/iqdemod.h:
    iqd_filter_*).  kind: "decimate_i16", "fir_i16", "fir_f32" or "iir_f32"; num: the taps (IIR: the numerator), den: the
    IIR's denominator without its leading 1 (None for the FIR kinds)."""
    KINDS = {"decimate_i16": 0, "fir_i16": 1, "fir_f32": 2, "iir_f32": 3}

    def __init__(self, engine, kind, num, den=None, factor=1, n_channels=1):
        self.kind, self.n_ch = self.KINDS.get(kind, kind), int(n_channels)
        self.dtype = np.int16 if self.kind in (0, 1) else np.float32
        num = None if num is None else np.ascontiguousarray(num, np.float32)
        den = None if den is None else np.ascontiguousarray(den, np.float32)
        self._create(engine, "filter", int(self.kind), _np_ptr(num), 0 if num is None else len(num),
                     _np_ptr(den), 0 if den is None else len(den), int(factor), self.n_ch)

    def out_count(self, n_in):
        return int(self._L.iqd_filter_out_count(self._h, int(n_in)))

    def run(self, x):
        """[n_channels, n_in] host array (or one row) -> [n_channels, out_count(n_in)]"""
        x = np.ascontiguousarray(x, self.dtype).reshape(self.n_ch, -1)
        out = np.zeros((self.n_ch, self.out_count(x.shape[1])), self.dtype)
        self._e._check(self._L.iqd_filter_run(self._h, _ptr_or_placeholder(x), x.shape[1], _ptr_or_placeholder(out)))
        return out

    def run_device(self, in_dev, n_in, out_dev):
        """iqd_filter_run_device: device pointers (integers), queued on the engine's stream."""
        self._e._check(self._L.iqd_filter_run_device(self._h, _dev_ptr(in_dev), int(n_in), _dev_ptr(out_dev)))

    def reset(self):
        self._e._check(self._L.iqd_filter_reset(self._h))


def filter_tile_samples(kind, n_num, n_den=0, factor=1):
    """iqd_filter_tile_samples (host only): the input samples (IIR: time steps) one workgroup stages per tile, 0 if out of range."""
    return int(_lib().iqd_filter_tile_samples(int(Filter.KINDS.get(kind, kind)), int(n_num), int(n_den), int(factor)))


def filter_clamp_free_taps(taps):
    """iqd_filter_clamp_free_taps (host only): how many leading taps, once quantised to Q15, can never reach the per-MAC clamp."""
    taps = np.ascontiguousarray(taps, np.float32)
    return int(_lib().iqd_filter_clamp_free_taps(_np_ptr(taps), len(taps)))


def channelizer_phasor_table():
    """The channelizer's phasor table P[i] = (c, s), [4096, 2] int16 (host only, no GPU)."""
    out = np.zeros(8192, np.int16)
    _ok(_lib().iqd_channelizer_phasor_table(_np_ptr(out)), "iqd_channelizer_phasor_table")
    return out.reshape(4096, 2)


def channelizer_default_taps(decimation, den=1):
    """The library's default Q15 prototype for decimation M, or for the fractional decimation / den (the prototype at
    the rate 256000 decimation, quantised per branch) (host only, no GPU)."""
    if int(den) == 1:
        ask, which = _lib().iqd_channelizer_default_taps, (int(decimation),)
    else:
        ask, which = _lib().iqd_channelizer_default_taps_q, (int(decimation), int(den))
    n = ask(*which, None, 0)
    if n < 0:
        raise IqdError(n, "no default taps for decimation %r / %r" % (decimation, den))
    out = np.zeros(n, np.int16)
    ask(*which, _np_ptr(out), n)
    return out


def channelizer_tuning(decimation, source_centre_hz, station_hz, rotation=1):
    """iqd_channelizer_tuning (host only): the increment that cuts station_hz + 64000 rotation out of a source centred on
    source_centre_hz at decimation x 256 kS/s, or None when that is out of band.  A bad decimation (2..64) or rotation
    (-1, 0, +1) raises IqdError, as the C function's IQD_EINVAL would otherwise read as "out of band"."""
    if not 2 <= int(decimation) <= 64 or int(rotation) not in (-1, 0, 1):
        raise IqdError(-1, "channelizer_tuning: decimation must be 2..64 and rotation -1, 0 or +1")
    inc = C.c_uint32()
    rc = _lib().iqd_channelizer_tuning(int(decimation), int(source_centre_hz), int(station_hz), int(rotation), C.byref(inc))
    if rc == -1:
        return None
    _ok(rc, "iqd_channelizer_tuning")
    return inc.value


def magnitude_dbfs(m):
    """iqd_magnitude_dbfs (host only): the squelch's level of a block magnitude, before any gain is subtracted."""
    return int(_lib().iqd_magnitude_dbfs(int(m)))


def phase_inc(offset_hz, fs):
    """The channelizer's phase increment for a channel at offset_hz from the capture's centre (f = int32(d) / 2^32 fs)."""
    return int(round(float(offset_hz) / float(fs) * 2.0 ** 32)) & 0xffffffff


_phase_inc = phase_inc      # (methods below take a `phase_inc` argument of their own)

# iqd_channelizer_config.sample_format: name -> (IQD_WIDE_*, the dtype of one rail; int16 is little-endian)
SAMPLE_FORMAT = {"u8": (0, np.dtype(np.uint8)), "s8": (1, np.dtype(np.int8)), "s16": (2, np.dtype("<i2"))}


def channelizer_window_outputs(decimation, n_taps, sample_format="u8"):
    """iqd_channelizer_window_outputs (host only): the most outputs per channel of one workgroup window, 0 if out of range."""
    return int(_lib().iqd_channelizer_window_outputs(int(decimation), int(n_taps), SAMPLE_FORMAT[sample_format][0]))


def channelizer_track_window_outputs(decimation, n_taps):
    """iqd_channelizer_track_window_outputs (host only): the most outputs of one window of a track follower's block."""
    return int(_lib().iqd_channelizer_track_window_outputs(int(decimation), int(n_taps)))


class _CaptureChild(_EngineChild):
    """An _EngineChild that reads n_sources wideband captures of one sample format; _what names it in messages."""
    _what = None

    def _set_format(self, sample_format):
        if sample_format not in SAMPLE_FORMAT:
            raise ValueError("sample_format must be one of %s" % ", ".join(SAMPLE_FORMAT))
        self.sample_format = sample_format
        self._code, self._dtype = SAMPLE_FORMAT[sample_format]

    def _capture(self, wide):
        """One call's capture as [n_sources, bytes_per_source] bytes.  An array of another sample format's dtype is a
        TypeError: a "u8" object refuses int8 / int16 arrays, "s8" and "s16" anything but their own dtype."""
        dt = getattr(wide, "dtype", None)
        if dt is not None and dt != self._dtype and (self._code != 0 or dt in (np.dtype(np.int8), np.dtype(np.int16))):
            raise TypeError("a %s of sample_format %r takes %s arrays, not %s" % (self._what, self.sample_format, self._dtype, dt))
        wide = np.ascontiguousarray(wide, dtype=self._dtype).reshape(self.n_sources, -1)
        return wide.view(np.uint8)


class Channelizer(_CaptureChild):
    """iqd_channelizer_*: n_channels channels cut out of n_sources wideband captures at decimation / decimation_den x
    256 kS/s (decimation_den 1, 2, 4 or 8; 2.4 MS/s is 75 / 8).  sample_format: what the captures hold - "u8" (offset
    binary, the RTL-SDR's), "s8" (int8) or "s16" (little-endian int16); run and accept_wideband then take
    [n_sources, 2 samples] arrays of that dtype."""
    _what = "channelizer"

    def __init__(self, engine, decimation, n_channels, n_sources=1, taps=None, decimation_den=1, sample_format="u8"):
        self._set_format(sample_format)
        self.rail_bytes = self._dtype.itemsize
        self.decimation, self.n_channels, self.n_sources = int(decimation), int(n_channels), int(n_sources)
        self.decimation_den = int(decimation_den) or 1
        self.n_points = 0                                        # survey points (set_survey)
        self._taps = None if taps is None else np.ascontiguousarray(taps, np.int16)
        cfg = ChannelizerConfig(self.n_sources, self.n_channels, self.decimation,
                                0 if self._taps is None else len(self._taps),
                                None if self._taps is None else self._taps.ctypes.data, int(decimation_den), self._code)
        self._create(engine, "channelizer", C.byref(cfg))

    def _range(self, first, n):
        return int(first), (self.n_channels - int(first) if n is None else int(n))

    def set_channels(self, first=0, source=None, offset_hz=None, fs=None, phase_inc=None, gain_shift=None, n=None):
        """Retunes channels [first, first + n): offsets in Hz with the capture's rate fs, or raw increments; a field left
        None keeps its value."""
        if offset_hz is not None:
            phase_inc = [_phase_inc(f, fs) for f in np.atleast_1d(offset_hz)]
        arrs = [None if v is None else np.atleast_1d(np.asarray(v)) for v in (source, phase_inc, gain_shift)]
        if n is None:
            n = max(len(a) for a in arrs if a is not None)
        src = None if arrs[0] is None else np.ascontiguousarray(np.broadcast_to(arrs[0], n), np.uint32)
        inc = None if arrs[1] is None else np.ascontiguousarray(np.broadcast_to(arrs[1].astype(np.uint64) & 0xffffffff, n), np.uint32)
        sh = None if arrs[2] is None else np.ascontiguousarray(np.broadcast_to(arrs[2], n), np.uint8)
        self._e._check(self._L.iqd_channelizer_set_channels(self._h, int(first), int(n), _np_ptr(src), _np_ptr(inc),
                                                            _np_ptr(sh)))

    def run(self, wide_u8):
        """[n_sources, bytes_per_source] uint8 -> [n_channels, bytes_per_source decimation_den / decimation] uint8 (host
        arrays).  sample_format "s8" / "s16": [n_sources, 2 samples] int8 / int16 -> [n_channels, 2 samples / decimation]."""
        wide = self._capture(wide_u8)
        out = np.zeros((self.n_channels, wide.shape[1] // (self.decimation * self.rail_bytes) * self.decimation_den), np.uint8)
        self._e._check(self._L.iqd_channelizer_run(self._h, _np_ptr(wide), wide.shape[1], _np_ptr(out)))
        return out

    def run_device(self, wide_dev, bytes_per_source, out_dev):
        self._e._check(self._L.iqd_channelizer_run_device(self._h, C.c_void_p(wide_dev), int(bytes_per_source),
                                                          C.c_void_p(out_dev)))

    def set_survey(self, offset_hz=None, fs=None, phase_inc=None, gain_shift=None):
        """The survey's points, measured on every source: offsets in Hz with the capture's rate fs, or raw increments;
        gain_shift one value or one per point (default 0).  No points (an empty list) clears the survey."""
        if offset_hz is not None:
            phase_inc = [_phase_inc(f, fs) for f in np.atleast_1d(offset_hz)]
        inc = np.atleast_1d(np.asarray([] if phase_inc is None else phase_inc))
        inc = np.ascontiguousarray(inc.astype(np.uint64) & 0xffffffff, np.uint32)
        sh = None if gain_shift is None else np.ascontiguousarray(np.broadcast_to(np.atleast_1d(np.asarray(gain_shift)), len(inc)), np.uint8)
        self._e._check(self._L.iqd_channelizer_set_survey(self._h, len(inc), _np_ptr(inc) if len(inc) else None,
                                                          _np_ptr(sh) if sh is not None and len(inc) else None))
        self.n_points = len(inc)

    def survey(self, wide_u8, block_bytes):
        """[n_sources, bytes_per_source] uint8 -> [n_sources, n_blocks, n_points] uint32: per block of block_bytes row
        bytes, the magnitude the squelch would see on each survey point.  Advances nothing."""
        wide = np.ascontiguousarray(wide_u8, dtype=np.uint8).reshape(self.n_sources, -1)
        block_bytes = int(block_bytes)
        row = wide.shape[1] // self.decimation * self.decimation_den
        out = np.zeros((self.n_sources, row // block_bytes if block_bytes > 0 else 0, self.n_points), np.uint32)
        self._e._check(self._L.iqd_channelizer_survey(self._h, _np_ptr(wide), wide.shape[1], block_bytes & 0xffffffff, _ptr_or_placeholder(out)))
        return out

    def survey_device(self, wide_dev, bytes_per_source, block_bytes, magnitude_dev):
        """iqd_channelizer_survey_device: device pointers (integers), queued on the engine's stream."""
        self._e._check(self._L.iqd_channelizer_survey_device(self._h, C.c_void_p(wide_dev), int(bytes_per_source),
                                                             int(block_bytes), C.c_void_p(magnitude_dev)))

    def reset(self):
        self._e._check(self._L.iqd_channelizer_reset(self._h))

    def set_source_frequency(self, centre_hz, first=0):
        """Centre frequencies (Hz) of sources [first, first + len)."""
        c = np.ascontiguousarray(np.atleast_1d(np.asarray(centre_hz, dtype=np.uint64)))
        self._e._check(self._L.iqd_channelizer_set_source_frequency(self._h, int(first), len(c), _np_ptr(c)))

    def follow_scanner(self, follow=True, first=0, n=None):
        """Channels [first, first + n) follow (or stop following) their engine channel's scanner."""
        self._e._check(self._L.iqd_channelizer_follow_scanner(self._h, *self._range(first, n), 1 if follow else 0))

    def follow_gain(self, follow=True, first=0, n=None):
        """Channels [first, first + n) follow (or stop following) their engine channel's IF gain: the channelizer applies it,
        in dB and per engine block, in place of the channel's gain shift."""
        self._e._check(self._L.iqd_channelizer_follow_gain(self._h, *self._range(first, n), 1 if follow else 0))

    def follow_tracks(self, slot, first=0, n=None):
        """Channels [first, first + n) follow slot[i] of their source's track table row (one value: all the same slot);
        -1 or None: they stop following."""
        s = None if slot is None else np.atleast_1d(np.asarray(slot, dtype=np.int64))
        first, n = self._range(first, len(s) if n is None and np.ndim(slot) else n)
        if s is not None:
            s = np.ascontiguousarray(np.clip(np.broadcast_to(s, n), -2 ** 31, 2 ** 31 - 1), np.int32)
        self._e._check(self._L.iqd_channelizer_follow_tracks(self._h, first, n, _np_ptr(s)))

    def set_track_table(self, slots_dev, n_slots=0, n_blocks=0, block_bytes=0, lag=0, min_state=2, reserved=(0, 0, 0)):
        """The track table the followers read: slots_dev a device pointer (integer) to [n_sources][n_blocks][n_slots]
        iqd_track_slot, as Tracker.run_device writes it; block_bytes the row bytes one table block covers.  None clears."""
        if slots_dev is None:
            self._e._check(self._L.iqd_channelizer_set_track_table(self._h, None))
            return
        t = TrackFollow(int(slots_dev) or None, int(n_slots), int(n_blocks), int(block_bytes), int(lag), int(min_state),
                        (C.c_uint32 * 3)(*[int(r) for r in reserved]))
        self._e._check(self._L.iqd_channelizer_set_track_table(self._h, C.byref(t)))


def spectrum_default_window(n_bins):
    """iqd_spectrum_default_window (host only, no GPU): the integer Hann window of n_bins entries, int16."""
    out = np.zeros(int(n_bins) if 0 < int(n_bins) <= 4096 else 1, np.int16)
    _ok(_lib().iqd_spectrum_default_window(int(n_bins) & 0xffffffff, _np_ptr(out)), "iqd_spectrum_default_window: n_bins %r" % (n_bins,))
    return out


def spectrum_full_scale(n_bins, window=None):
    """iqd_spectrum_full_scale (host only, no GPU): the power of bin n_bins / 2 for the constant U8 input (255, 128)."""
    w = None if window is None else np.ascontiguousarray(window, np.int16)
    if w is not None and len(w) != int(n_bins):
        raise ValueError("the window must have n_bins (%d) entries, not %d" % (int(n_bins), len(w)))
    p = C.c_uint32()
    _ok(_lib().iqd_spectrum_full_scale(_np_ptr(w), int(n_bins) & 0xffffffff, C.byref(p)),
        "iqd_spectrum_full_scale: n_bins %r or the window out of range" % (n_bins,))
    return p.value


def spectrum_dbfs(power, p_fs):
    """10 log10(max(power, 1) / p_fs): a power of Spectrum.run against spectrum_full_scale, in dBFS (float64)."""
    return 10.0 * np.log10(np.maximum(np.asarray(power, np.float64), 1.0) / float(p_fs))


class Spectrum(_CaptureChild):
    """iqd_spectrum_*: the integer periodogram of n_sources wideband captures, n_bins bins (64 .. 2048, a power of two) from
    low to high frequency, the centre frequency at bin n_bins / 2.  window: n_bins int16 values (None: the default Hann
    window); sample_format "u8" or "s8"."""
    _what = "spectrum"

    def __init__(self, engine, n_bins, n_sources=1, window=None, sample_format="u8"):
        self._set_format(sample_format)
        self.n_bins, self.n_sources = int(n_bins), int(n_sources)
        self._window = None if window is None else np.ascontiguousarray(window, np.int16)
        if self._window is not None and self._window.shape != (self.n_bins,):
            raise ValueError("the window must have n_bins (%d) entries" % self.n_bins)
        cfg = SpectrumConfig(self.n_sources & 0xffffffff, self.n_bins & 0xffffffff,
                             None if self._window is None else self._window.ctypes.data, self._code)
        self._create(engine, "spectrum", C.byref(cfg))

    def run(self, wide, frames_per_block):
        """[n_sources, bytes_per_source] of the format's dtype -> [n_sources, n_blocks, n_bins] uint32 (host arrays),
        n_blocks = bytes_per_source / (2 n_bins frames_per_block)."""
        wide = self._capture(wide)
        F = int(frames_per_block)
        nb = wide.shape[1] // (2 * self.n_bins * F) if F > 0 else 0
        out = np.zeros((self.n_sources, nb, self.n_bins), np.uint32)
        self._e._check(self._L.iqd_spectrum_run(self._h, _ptr_or_placeholder(wide), wide.shape[1], F & 0xffffffff, _ptr_or_placeholder(out)))
        return out

    def run_device(self, wide_dev, bytes_per_source, frames_per_block, power_dev):
        """iqd_spectrum_run_device: device pointers (integers), queued on the engine's stream."""
        self._e._check(self._L.iqd_spectrum_run_device(self._h, _dev_ptr(wide_dev), int(bytes_per_source),
                                                       int(frames_per_block) & 0xffffffff, _dev_ptr(power_dev)))


def detect_offset_hz(n_bins, rate_hz, centroid_q8):
    """iqd_detect_offset_hz (host only, no GPU): a detection's centroid as the offset in Hz from the capture's centre,
    floor(((centroid_q8 - 128 N) rate + 128 N) / (256 N)) - what channelizer_tuning takes as station - centre."""
    return _u32_function("iqd_detect_offset_hz", C.c_int64(), (n_bins, rate_hz, centroid_q8),
                         "iqd_detect_offset_hz: n_bins %r, rate_hz %r or centroid_q8 %r out of range" % (n_bins, rate_hz, centroid_q8))


class Detector(_EngineChild):
    """iqd_detect_*: the occupied runs of band spectrum rows of n_bins bins (64 .. 2048, a power of two).  floor_rank: which
    of the row's sorted values is the noise floor (None: n_bins / 2, the upper median); ratio_q8: the threshold over it
    (256 = 1.0); dc_guard: bins N / 2 - d < k < N / 2 + d never count; bridge: the gap two hot bins of one run may have;
    min_width: narrower runs are dropped; max_detections: records per row."""

    def __init__(self, engine, n_bins, floor_rank=None, ratio_q8=2048, dc_guard=1, bridge=8, min_width=3, max_detections=16):
        self.n_bins, self.max_detections = int(n_bins), int(max_detections)
        rank = self.n_bins // 2 if floor_rank is None else int(floor_rank)
        cfg = _u32_config(DetectConfig, (n_bins, rank, ratio_q8, dc_guard, bridge, min_width, max_detections))
        self._create(engine, "detect", C.byref(cfg))

    def run(self, power):
        """[..., n_bins] uint32 (host array; a Spectrum.run result as it is) -> (rows [n_rows] DETECT_ROW,
        det [n_rows, max_detections] DETECTION), n_rows the product of the leading dimensions."""
        if getattr(power, "dtype", None) != np.uint32:
            raise TypeError("the power rows are uint32, not %s" % getattr(power, "dtype", type(power)))
        power = np.ascontiguousarray(power).reshape(-1, self.n_bins)
        rows = np.zeros(len(power), DETECT_ROW)
        det = np.zeros((len(power), self.max_detections), DETECTION)
        self._e._check(self._L.iqd_detect_run(self._h, _ptr_or_placeholder(power), len(power), _ptr_or_placeholder(rows), _ptr_or_placeholder(det)))
        return rows, det

    def run_device(self, power_dev, n_rows, rows_dev, det_dev):
        """iqd_detect_run_device: device pointers (integers), queued on the engine's stream."""
        self._e._check(self._L.iqd_detect_run_device(self._h, _dev_ptr(power_dev), int(n_rows), _dev_ptr(rows_dev), _dev_ptr(det_dev)))

    def offset_hz(self, rate_hz, centroid_q8):
        """detect_offset_hz for this detector's n_bins"""
        return detect_offset_hz(self.n_bins, rate_hz, centroid_q8)


def track_phase_inc(n_bins, centroid_q8, inc_bias=0):
    """iqd_track_phase_inc (host only, no GPU): the channelizer phase_inc of a centre in 1/256 bins,
    (uint32)((centroid_q8 - 128 N) 2^(24 - log2 N)) + inc_bias mod 2^32 - what Channelizer.set_channels takes."""
    return _u32_function("iqd_track_phase_inc", C.c_uint32(), (n_bins, centroid_q8, inc_bias),
                         "iqd_track_phase_inc: n_bins %r or centroid_q8 %r out of range" % (n_bins, centroid_q8))


def track_default_edges(n_bins):
    """the width classes used where none are given: runs of at least 1/64, 1/16 and 1/4 of the band (and of 2 bins)"""
    n = int(n_bins)
    return (max(n // 64, 1) + 1, max(n // 16, 2), max(n // 4, 2))


class Tracker(_EngineChild):
    """iqd_track_*: the detector's runs followed from block to block - n_slots fixed slots per source, each a track with a
    persistent id, hysteresis (open after open_hits hits, held over hold_blocks misses), a centre smoothed by alpha_q8 / 256,
    its exact phase_inc (plus inc_bias) and a width class (class_edge: three widths in bins).  n_bins and max_detections
    are the Detector's.  State is carried from call to call until reset()."""

    def __init__(self, engine, n_bins, n_sources=1, max_detections=16, n_slots=8, gate_q8=512, open_hits=3, hold_blocks=2,
                 alpha_q8=64, inc_bias=0, class_edge=None):
        self.n_bins, self.n_sources, self.max_detections, self.n_slots = int(n_bins), int(n_sources), int(max_detections), int(n_slots)
        edges = track_default_edges(n_bins) if class_edge is None else tuple(int(v) for v in class_edge)
        if len(edges) != 3:
            raise ValueError("class_edge must have three entries")
        cfg = _u32_config(TrackConfig, (n_sources, n_bins, max_detections, n_slots, gate_q8, open_hits, hold_blocks, alpha_q8, inc_bias),
                          class_edge=edges)
        self._create(engine, "track", C.byref(cfg))

    def run(self, rows, det):
        """rows [n_sources, n_blocks] DETECT_ROW and det [n_sources, n_blocks, max_detections] DETECTION (host arrays; a
        Detector.run result reshaped) -> (slots [n_sources, n_blocks, n_slots] TRACK_SLOT, blocks [n_sources, n_blocks]
        TRACK_BLOCK)."""
        if getattr(rows, "dtype", None) != DETECT_ROW or getattr(det, "dtype", None) != DETECTION:
            raise TypeError("rows are DETECT_ROW and det DETECTION arrays")
        rows = np.ascontiguousarray(rows).reshape(self.n_sources, -1)
        nb = rows.shape[1]
        det = np.ascontiguousarray(det).reshape(self.n_sources, nb, self.max_detections)
        slots = np.zeros((self.n_sources, nb, self.n_slots), TRACK_SLOT)
        blocks = np.zeros((self.n_sources, nb), TRACK_BLOCK)
        self._e._check(self._L.iqd_track_run(self._h, _ptr_or_placeholder(rows), _ptr_or_placeholder(det), nb, _ptr_or_placeholder(slots),
                                             _ptr_or_placeholder(blocks)))
        return slots, blocks

    def run_device(self, rows_dev, det_dev, n_blocks, slots_dev, blocks_dev):
        """iqd_track_run_device: device pointers (integers), queued on the engine's stream."""
        self._e._check(self._L.iqd_track_run_device(self._h, _dev_ptr(rows_dev), _dev_ptr(det_dev), int(n_blocks),
                                                    _dev_ptr(slots_dev), _dev_ptr(blocks_dev)))

    def reset(self):
        """iqd_track_reset: every slot free, ids count from 1 again."""
        self._e._check(self._L.iqd_track_reset(self._h))

    def state(self, source=0):
        """iqd_track_get_state: the source's n_slots slots as they stand after the last block (synchronises)."""
        out = np.zeros(self.n_slots, TRACK_SLOT)
        if not 0 <= int(source) <= 0xffffffff:
            raise IqdError(-1, "iqd_track_get_state: source %r out of range" % (source,))
        self._e._check(self._L.iqd_track_get_state(self._h, int(source), _np_ptr(out)))
        return out


def measure_defaults(n_bins):
    """the thresholds used where none are given (DESIGN 4.15 has the measurements they were chosen from): a margin of
    N / 256 bins, 0.5 % of the power left outside at each end, a carrier of the peak bin and one on each side, no hint under
    a sum of 4096, CARRIER from 160 / 256 of the power in the carrier, WIDE from an occupied band of N / 32 bins"""
    n = int(n_bins)
    return dict(margin=max(n // 256, 1), obw_tail_q16=328, carrier_half=1, min_sum=4096, carrier_min_q8=160, wide_bins=max(n // 32, 2))


class Measure(_EngineChild):
    """iqd_measure_*: what every track of a Tracker's table is in a block - the excess power over the Detector's floor in the
    track's run widened by `margin` bins, the occupied bandwidth that leaves obw_tail_q16 / 65536 of it outside at each end,
    the share of it within carrier_half bins of the peak, and a mode hint (HINT_*) from wide_bins and carrier_min_q8.
    n_bins and dc_guard are the Detector's, n_slots the Tracker's.  Stateless."""

    def __init__(self, engine, n_bins, n_sources=1, n_slots=8, dc_guard=1, margin=None, obw_tail_q16=None, carrier_half=None,
                 min_sum=None, carrier_min_q8=None, wide_bins=None, reserved=(0, 0)):
        self.n_bins, self.n_sources, self.n_slots = int(n_bins), int(n_sources), int(n_slots)
        given = dict(margin=margin, obw_tail_q16=obw_tail_q16, carrier_half=carrier_half, min_sum=min_sum,
                     carrier_min_q8=carrier_min_q8, wide_bins=wide_bins)
        v = dict(measure_defaults(n_bins), **{k: x for k, x in given.items() if x is not None})
        cfg = _u32_config(MeasureConfig, (n_sources, n_bins, n_slots, dc_guard, v["margin"], v["obw_tail_q16"], v["carrier_half"],
                                          v["min_sum"], v["carrier_min_q8"], v["wide_bins"]), reserved=reserved)
        self._create(engine, "measure", C.byref(cfg))

    def run(self, power, rows, slots):
        """power [n_sources, n_blocks, n_bins] uint32, rows [n_sources, n_blocks] DETECT_ROW, slots [n_sources, n_blocks,
        n_slots] TRACK_SLOT (host arrays: Spectrum.run's, Detector.run's and Tracker.run's) -> [n_sources, n_blocks, n_slots]
        TRACK_MEASURE."""
        if getattr(power, "dtype", None) != np.uint32 or getattr(rows, "dtype", None) != DETECT_ROW or getattr(slots, "dtype", None) != TRACK_SLOT:
            raise TypeError("power is uint32, rows are DETECT_ROW and slots TRACK_SLOT arrays")
        rows = np.ascontiguousarray(rows).reshape(self.n_sources, -1)
        nb = rows.shape[1]
        power = np.ascontiguousarray(power).reshape(self.n_sources, nb, self.n_bins)
        slots = np.ascontiguousarray(slots).reshape(self.n_sources, nb, self.n_slots)
        meas = np.zeros((self.n_sources, nb, self.n_slots), TRACK_MEASURE)
        self._e._check(self._L.iqd_measure_run(self._h, _ptr_or_placeholder(power), _ptr_or_placeholder(rows), _ptr_or_placeholder(slots), nb,
                                               _ptr_or_placeholder(meas)))
        return meas

    def run_device(self, power_dev, rows_dev, slots_dev, n_blocks, meas_dev):
        """iqd_measure_run_device: device pointers (integers), queued on the engine's stream."""
        self._e._check(self._L.iqd_measure_run_device(self._h, _dev_ptr(power_dev), _dev_ptr(rows_dev),
                                                      _dev_ptr(slots_dev), int(n_blocks), _dev_ptr(meas_dev)))


def tracklog_defaults():
    """the settings used where none are given: a track is an event from two active blocks on, a mode is decided from four
    votes on, and a call keeps up to 256 events per source"""
    return dict(min_active=2, vote_min=4, max_events=256)


def tracklog_mean_centre(sum_centre_q8, n_active):
    """iqd_tracklog_mean_centre (host only, no GPU): floor(sum_centre_q8 / n_active), a track's mean centre in 1/256 bins -
    what detect_offset_hz and track_phase_inc take."""
    return _u32_function("iqd_tracklog_mean_centre", C.c_uint32(), (sum_centre_q8, n_active),
                         "iqd_tracklog_mean_centre: sum_centre_q8 %r or n_active %r out of range" % (sum_centre_q8, n_active), bits=64)


class TrackLog(_EngineChild):
    """iqd_tracklog_*: a running summary of every (source, slot) of a Tracker's table over its track's whole life - blocks
    seen and active, the mean centre's sum, the measurements' extremes, a mode hint voted over every measured block - and one
    event record per track that ends with at least min_active active blocks.  n_slots is the Tracker's.  State is carried from
    call to call until reset()."""

    def __init__(self, engine, n_sources=1, n_slots=8, max_events=None, min_active=None, vote_min=None, reserved=(0, 0, 0)):
        self.n_sources, self.n_slots = int(n_sources), int(n_slots)
        given = dict(max_events=max_events, min_active=min_active, vote_min=vote_min)
        v = dict(tracklog_defaults(), **{k: x for k, x in given.items() if x is not None})
        self.max_events = int(v["max_events"])
        cfg = _u32_config(TrackLogConfig, (n_sources, n_slots, v["max_events"], v["min_active"], v["vote_min"]), reserved=reserved)
        self._create(engine, "tracklog", C.byref(cfg))

    def run(self, slots, meas):
        """slots [n_sources, n_blocks, n_slots] TRACK_SLOT and meas [n_sources, n_blocks, n_slots] TRACK_MEASURE (host arrays:
        Tracker.run's and Measure.run's) -> (summary [n_sources, n_blocks, n_slots] TRACK_SUMMARY, events [n_sources,
        max_events] TRACK_SUMMARY, counts [n_sources] TRACKLOG_COUNTS)."""
        if getattr(slots, "dtype", None) != TRACK_SLOT or getattr(meas, "dtype", None) != TRACK_MEASURE:
            raise TypeError("slots are TRACK_SLOT and meas TRACK_MEASURE arrays")
        slots = np.ascontiguousarray(slots).reshape(self.n_sources, -1, self.n_slots)
        nb = slots.shape[1]
        meas = np.ascontiguousarray(meas).reshape(self.n_sources, nb, self.n_slots)
        summary = np.zeros((self.n_sources, nb, self.n_slots), TRACK_SUMMARY)
        events = np.zeros((self.n_sources, self.max_events), TRACK_SUMMARY)
        counts = np.zeros(self.n_sources, TRACKLOG_COUNTS)
        self._e._check(self._L.iqd_tracklog_run(self._h, _ptr_or_placeholder(slots), _ptr_or_placeholder(meas), nb, _ptr_or_placeholder(summary),
                                                _np_ptr(events), _np_ptr(counts)))
        return summary, events, counts

    def run_device(self, slots_dev, meas_dev, n_blocks, summary_dev, events_dev, counts_dev):
        """iqd_tracklog_run_device: device pointers (integers), queued on the engine's stream."""
        self._e._check(self._L.iqd_tracklog_run_device(self._h, _dev_ptr(slots_dev), _dev_ptr(meas_dev), int(n_blocks),
                                                       _dev_ptr(summary_dev), _dev_ptr(events_dev), _dev_ptr(counts_dev)))

    def reset(self):
        """iqd_tracklog_reset: every summary free, block indices count from 0 again."""
        self._e._check(self._L.iqd_tracklog_reset(self._h))

    def state(self, source=0):
        """iqd_tracklog_get_state: (the source's n_slots summaries as they stand after the last block, its block index);
        synchronises."""
        out = np.zeros(self.n_slots, TRACK_SUMMARY)
        g = C.c_uint64()
        if not 0 <= int(source) <= 0xffffffff:
            raise IqdError(-1, "iqd_tracklog_get_state: source %r out of range" % (source,))
        self._e._check(self._L.iqd_tracklog_get_state(self._h, int(source), _np_ptr(out), C.byref(g)))
        return out, g.value
