"""Every refusal of the channelizer's host code (iqd_channelizer_*, iqd_accept_wideband*) as a table {label: [status, text]},
made through the raw library and through rtlsdrdiags_amd.capi wherever capi lets the call reach the library, at 2 sources,
4 channels, M = 8 and 512 capture bytes per source, on four objects (U8, the fractional 75 / 8, S8, S16 with 1024 bytes) and
two engines (4 channels with block_bytes 256, and 2 channels: "belongs to another engine" needs a second one).  A raw call
records iqd_last_error's text, a capi call the IqdError's; a call with a NULL object or engine, and a host-only function, must
leave the engine's last error as it was and records that.  Double faults pin which refusal wins.  (IQD_WIDE_S16 together with
a fractional rate cannot be made: create refuses the pair, and that refusal is in the table.)

Around the table every object makes one valid run before it and one after it: the two outputs together must be the model's
rows of the two captures concatenated, so no refused call moved the history, the output count or a channel's kind.  Nothing
else is launched.

tests/golden/chan_refusals.json is this table as the library gave it before csrc/iqd_chan.cpp was cut into one file per
concern:  python -m tests.chan_refusals tests/golden/chan_refusals.json  (on the GPU)."""
import ctypes as C
import json
import sys

import numpy as np

from tests import chan_frac_model as cfm
from tests import chan_model as cm

SRC, NCH, M, BPS = 2, 4, 8, 512
FP, FQ, FBPS = 75, 8, 64 * 75                          # the fractional object and its shortest capture
UNTOUCHED = "(last error untouched)"
CH_SRC, CH_INC, CH_SHIFT = [0, 1, 1, 0], [0x10000000, 0xe0000000, 0x00300000, 0x7fffffff], [0, 3, 8, 1]
ROOM = 1 << 16                                          # bytes of every array: whatever a call names stays inside


def captures(seed):
    """the four objects' captures of one call, the same signal in each format where the rate allows"""
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, (SRC, BPS), dtype=np.uint8)
    return {"u8": u8, "s8": (u8 ^ 0x80).view(np.int8), "s16": ((u8.astype(np.int32) - 128) * 256).astype("<i2"),
            "frac": rng.integers(0, 256, (SRC, FBPS), dtype=np.uint8)}


def model(capi, first, second):
    """{object: the rows of both calls, [NCH, 2 row bytes]}; S8 and S16 of the same signal give U8's rows"""
    P = capi.channelizer_phasor_table()
    whole = cm.channelize(np.concatenate([first["u8"], second["u8"]], axis=1), capi.channelizer_default_taps(M), M, CH_SRC, CH_INC, CH_SHIFT, P)
    frac = cfm.channelize(np.concatenate([first["frac"], second["frac"]], axis=1), capi.channelizer_default_taps(FP, FQ), FP, FQ,
                          CH_SRC, CH_INC, CH_SHIFT, P)
    return {"u8": whole, "s8": whole, "s16": whole, "frac": frac}


def collect(capi):
    """-> dict(table={label: [status, text]}, rows={object: both valid runs' rows side by side}, want=model's)"""
    L = capi._lib()
    eng, eng2 = capi.Engine(NCH, block_bytes=256), capi.Engine(2)
    table = {}

    def put(label, entry):
        assert label not in table, label
        table[label] = entry

    def raw(label, fn, *args, untouched=False, on=None, **kw):
        on = on or eng
        before = L.iqd_last_error(on._h)
        rc = fn(*args, **kw)
        text = L.iqd_last_error(on._h).decode()
        put(label, [rc, UNTOUCHED if untouched and text == before.decode() else text])

    def wrapped(label, fn, *args, **kw):
        try:
            made = fn(*args, **kw)
        except capi.IqdError as err:
            put(label, [err.status, str(err)])
        else:
            put(label, [0, ""])
            if hasattr(made, "close"):
                made.close()

    def channelizer(e, **kw):
        z = capi.Channelizer(e, FP if kw.get("decimation_den") else M, NCH, n_sources=SRC, **kw)
        z.set_channels(0, source=CH_SRC, phase_inc=CH_INC, gain_shift=CH_SHIFT)
        return z

    objs = {"u8": channelizer(eng), "frac": channelizer(eng, decimation_den=FQ), "s8": channelizer(eng, sample_format="s8"),
            "s16": channelizer(eng, sample_format="s16")}
    zu, zf, z8, z16 = (objs[k] for k in ("u8", "frac", "s8", "s16"))
    z_other = channelizer(eng2)                         # four channels on the engine of two
    first, second = captures(1), captures(2)
    rows = {k: [z.run(first[k])] for k, z in objs.items()}

    host = {k: np.zeros(ROOM, np.uint8) for k in ("wide", "out", "pcm", "cnt", "mag", "sp")}
    hp = {k: v.ctypes.data for k, v in host.items()}
    dp = {k: eng.dev_alloc(ROOM) for k in ("wide", "out", "pcm", "cnt", "mag", "sp", "slots")}
    for p in dp.values():
        eng.dev_upload(p, np.zeros(ROOM, np.uint8))
    eng.synchronize()
    NULL, vp = None, C.c_void_p

    # ---- create -----------------------------------------------------------------------------------------------------------
    good = dict(n_sources=SRC, n_channels=NCH, decimation=M, n_taps=0, taps=None, decimation_den=0, sample_format=0)
    keep = []

    def config(reserved=None, **kw):
        v = dict(good, **kw)
        if v["taps"] is not None:
            keep.append(np.ascontiguousarray(v["taps"], np.int16))
            v["taps"], v["n_taps"] = keep[-1].ctypes.data, v["n_taps"] or len(keep[-1])
        cfg = capi.ChannelizerConfig(v["n_sources"], v["n_channels"], v["decimation"], v["n_taps"], v["taps"], v["decimation_den"],
                                     v["sample_format"])
        if reserved is not None:
            cfg.reserved[reserved] = 1
        return cfg

    h = vp()
    create = L.iqd_channelizer_create
    raw("create.raw.cfg NULL", create, eng._h, NULL, C.byref(h))
    raw("create.raw.out NULL", create, eng._h, C.byref(config()), NULL)
    raw("create.raw.cfg and out NULL", create, eng._h, NULL, NULL)
    raw("create.raw.engine NULL", create, NULL, C.byref(config()), C.byref(h), untouched=True)
    spike = lambda n, v: np.concatenate([np.full(1, v, np.int16), np.zeros(n - 1, np.int16)])
    fields = [
        ("n_sources=0", dict(n_sources=0)), ("n_channels=0", dict(n_channels=0)), ("decimation=0", dict(decimation=0)),
        ("decimation=1", dict(decimation=1)), ("decimation=65", dict(decimation=65)), ("decimation=65 den=1", dict(decimation=65, decimation_den=1)),
        ("den=3", dict(decimation_den=3)), ("den=5", dict(decimation=75, decimation_den=5)), ("den=16", dict(decimation=75, decimation_den=16)),
        ("den=2^32-1", dict(decimation_den=2 ** 32 - 1)), ("8/2 not coprime", dict(decimation=8, decimation_den=2)),
        ("74/8 not coprime", dict(decimation=74, decimation_den=8)), ("3/2 below 2", dict(decimation=3, decimation_den=2)),
        ("15/8 below 2", dict(decimation=15, decimation_den=8)), ("129/2 above 64", dict(decimation=129, decimation_den=2)),
        ("513/8 above 64", dict(decimation=513, decimation_den=8)), ("1/2", dict(decimation=1, decimation_den=2)),
        ("sample_format=3", dict(sample_format=3)), ("sample_format=2^32-1", dict(sample_format=2 ** 32 - 1)),
        ("s8 75/8", dict(decimation=FP, decimation_den=FQ, sample_format=1)), ("s16 75/8", dict(decimation=FP, decimation_den=FQ, sample_format=2)),
        ("s16 9/2", dict(decimation=9, decimation_den=2, sample_format=2)),
        ("n_taps=1025", dict(taps=np.ones(1025, np.int16))), ("75/8 n_taps=8193", dict(decimation=FP, decimation_den=FQ, taps=np.ones(8193, np.int16))),
        ("h[0]=32640", dict(taps=spike(9, 32640))), ("h[0]=-32640", dict(taps=spike(9, -32640))),
        ("75/8 h[0]=32640", dict(decimation=FP, decimation_den=FQ, taps=spike(9, 32640))),
        ("75/8 h[0]=-32640", dict(decimation=FP, decimation_den=FQ, taps=spike(9, -32640))),
        ("sum |h|", dict(taps=np.full(1024, 8192, np.int16))), ("sum |h| negative taps", dict(taps=np.full(1024, -8192, np.int16))),
        ("75/8 sum |h| of a branch", dict(decimation=FP, decimation_den=FQ, taps=np.full(8192, 8192, np.int16))),
        ("n_channels=2^20+1", dict(n_channels=2 ** 20 + 1)), ("n_sources=2^20+1", dict(n_sources=2 ** 20 + 1)),
        # two at once: the first of the list above wins
        ("n_sources=0 and sample_format=3", dict(n_sources=0, sample_format=3)), ("decimation=65 and den=3", dict(decimation=65, decimation_den=3)),
        ("den=3 and sample_format=3", dict(decimation_den=3, sample_format=3)), ("sample_format=3 and n_taps=1025", dict(sample_format=3, taps=np.ones(1025, np.int16))),
        ("n_taps=1025 and h[0]=32640", dict(taps=spike(1025, 32640))), ("h[0]=32640 and n_channels=2^20+1", dict(taps=spike(9, 32640), n_channels=2 ** 20 + 1)),
        ("s16 75/8 and n_channels=2^20+1", dict(decimation=FP, decimation_den=FQ, sample_format=2, n_channels=2 ** 20 + 1)),
    ]
    for label, kw in fields:
        raw("create.raw." + label, create, eng._h, C.byref(config(**kw)), C.byref(h))
    cfg = config(taps=np.ones(4, np.int16))
    cfg.n_taps = 0                                       # a tap pointer and no taps
    raw("create.raw.taps with n_taps=0", create, eng._h, C.byref(cfg), C.byref(h))
    cfg = config(decimation=FP, decimation_den=FQ, taps=np.ones(4, np.int16))
    cfg.n_taps = 0
    raw("create.raw.75/8 taps with n_taps=0", create, eng._h, C.byref(cfg), C.byref(h))
    for i in range(2):
        raw("create.raw.reserved[%d]" % i, create, eng._h, C.byref(config(reserved=i)), C.byref(h))
    raw("create.raw.den=3 and reserved[0]", create, eng._h, C.byref(config(reserved=0, decimation_den=3)), C.byref(h))
    raw("create.raw.reserved[1] and sample_format=3", create, eng._h, C.byref(config(reserved=1, sample_format=3)), C.byref(h))
    put("create.raw.handle", [0, "still NULL" if not h.value else "set"])
    for label, args, kw in (("decimation=65", (65, NCH), {}), ("decimation=1", (1, NCH), {}), ("n_channels=0", (M, 0), {}),
                            ("n_sources=0", (M, NCH), dict(n_sources=0)), ("den=3", (M, NCH), dict(decimation_den=3)),
                            ("8/2 not coprime", (8, NCH), dict(decimation_den=2)), ("s8 75/8", (FP, NCH), dict(decimation_den=FQ, sample_format="s8")),
                            ("s16 75/8", (FP, NCH), dict(decimation_den=FQ, sample_format="s16")), ("n_taps=1025", (M, NCH), dict(taps=np.ones(1025, np.int16))),
                            ("75/8 n_taps=8193", (FP, NCH), dict(decimation_den=FQ, taps=np.ones(8193, np.int16))),
                            ("h[0]=32640", (M, NCH), dict(taps=spike(9, 32640))), ("sum |h|", (M, NCH), dict(taps=np.full(1024, 8192, np.int16))),
                            ("75/8 sum |h| of a branch", (FP, NCH), dict(decimation_den=FQ, taps=np.full(8192, 8192, np.int16))),
                            ("n_channels=2^20+1", (M, 2 ** 20 + 1), {})):
        wrapped("create.capi." + label, capi.Channelizer, eng, *args, **kw)

    # ---- set_channels, set_source_frequency, set_survey ---------------------------------------------------------------------
    u32 = lambda *v: np.array(v, np.uint32)
    u8a = lambda *v: np.array(v, np.uint8)
    setc = L.iqd_channelizer_set_channels
    raw("set_channels.raw.object NULL", setc, NULL, 0, 1, NULL, NULL, NULL, untouched=True)
    for label, f, n in (("n=0", 0, 0), ("first=4", NCH, 1), ("first=3 n=2", 3, 2), ("n=2^32-1", 1, 2 ** 32 - 1), ("first=2^32-1", 2 ** 32 - 1, 1)):
        raw("set_channels.raw." + label, setc, zu._h, f, n, NULL, NULL, NULL)
    raw("set_channels.raw.source=2", setc, zu._h, 0, 2, capi._np_ptr(u32(1, SRC)), NULL, NULL)
    raw("set_channels.raw.gain_shift=9", setc, zu._h, 0, 2, NULL, NULL, capi._np_ptr(u8a(8, 9)))
    raw("set_channels.raw.source=2 and gain_shift=9", setc, zu._h, 0, 1, capi._np_ptr(u32(SRC)), NULL, capi._np_ptr(u8a(9)))
    raw("set_channels.raw.gain_shift[0]=9 and source[1]=2", setc, zu._h, 0, 2, capi._np_ptr(u32(0, SRC)), NULL, capi._np_ptr(u8a(9, 0)))
    raw("set_channels.raw.first=4 and source=2", setc, zu._h, NCH, 1, capi._np_ptr(u32(SRC)), NULL, NULL)
    wrapped("set_channels.capi.first=4", zu.set_channels, NCH, source=[0])
    wrapped("set_channels.capi.first=3 n=2", zu.set_channels, 3, source=[0, 0])
    wrapped("set_channels.capi.source=2", zu.set_channels, 0, source=[SRC])
    wrapped("set_channels.capi.gain_shift=9", zu.set_channels, 0, gain_shift=[9])
    setf = L.iqd_channelizer_set_source_frequency
    hz = np.array([100000000, 101000000], np.uint64)
    raw("set_source_frequency.raw.object NULL", setf, NULL, 0, 1, capi._np_ptr(hz), untouched=True)
    raw("set_source_frequency.raw.centre NULL", setf, zu._h, 0, 1, NULL)
    for label, f, n in (("n=0", 0, 0), ("first=2", SRC, 1), ("first=1 n=2", 1, 2), ("n=2^32-1", 1, 2 ** 32 - 1)):
        raw("set_source_frequency.raw." + label, setf, zu._h, f, n, capi._np_ptr(hz))
    wrapped("set_source_frequency.capi.first=2", zu.set_source_frequency, [1], first=SRC)
    wrapped("set_source_frequency.capi.first=1 n=2", zu.set_source_frequency, [1, 2], first=1)
    sets = L.iqd_channelizer_set_survey
    pts = np.arange(4097, dtype=np.uint32) << 16
    raw("set_survey.raw.object NULL", sets, NULL, 1, capi._np_ptr(pts), NULL, untouched=True)
    raw("set_survey.raw.n_points=4097", sets, zu._h, 4097, capi._np_ptr(pts), NULL)
    raw("set_survey.raw.s16", sets, z16._h, 1, capi._np_ptr(pts), NULL)
    raw("set_survey.raw.s8", sets, z8._h, 1, capi._np_ptr(pts), NULL)
    raw("set_survey.raw.increments NULL", sets, zu._h, 1, NULL, NULL)
    raw("set_survey.raw.gain_shift=9", sets, zu._h, 2, capi._np_ptr(pts), capi._np_ptr(u8a(0, 9)))
    raw("set_survey.raw.s16 and n_points=4097", sets, z16._h, 4097, capi._np_ptr(pts), NULL)
    raw("set_survey.raw.s8 and increments NULL", sets, z8._h, 1, NULL, NULL)
    raw("set_survey.raw.increments NULL and gain_shift=9", sets, zu._h, 1, NULL, capi._np_ptr(u8a(9)))
    wrapped("set_survey.capi.n_points=4097", zu.set_survey, phase_inc=pts)
    wrapped("set_survey.capi.s16", z16.set_survey, phase_inc=[0])
    wrapped("set_survey.capi.s8", z8.set_survey, phase_inc=[0])
    wrapped("set_survey.capi.gain_shift=9", zu.set_survey, phase_inc=[0, 1], gain_shift=[0, 9])

    # ---- follow_scanner, follow_gain, follow_tracks, set_track_table ---------------------------------------------------------
    i32 = lambda *v: np.array(v, np.int32)
    fs, fg, ft = L.iqd_channelizer_follow_scanner, L.iqd_channelizer_follow_gain, L.iqd_channelizer_follow_tracks
    RANGES = (("n=0", 0, 0), ("first=4", NCH, 1), ("first=3 n=2", 3, 2), ("n=2^32-1", 1, 2 ** 32 - 1))
    for name, fn, meth in (("follow_scanner", fs, "follow_scanner"), ("follow_gain", fg, "follow_gain")):
        raw(name + ".raw.object NULL", fn, NULL, 0, 1, 1, untouched=True)
        for label, f, n in RANGES:
            raw("%s.raw.%s" % (name, label), fn, zu._h, f, n, 1)
            raw("%s.raw.stop %s" % (name, label), fn, zu._h, f, n, 0)
        wrapped(name + ".capi.first=4", getattr(zu, meth), True, NCH, 1)
        for k in ("s16", "s8", "frac"):
            raw("%s.raw.%s" % (name, k), fn, objs[k]._h, 0, 1, 1)
            raw("%s.raw.%s and first=4" % (name, k), fn, objs[k]._h, NCH, 1, 1)
            wrapped("%s.capi.%s" % (name, k), getattr(objs[k], meth), True, 0, 1)
    raw("follow_tracks.raw.object NULL", ft, NULL, 0, 1, capi._np_ptr(i32(0)), untouched=True)
    for label, f, n in RANGES:
        raw("follow_tracks.raw." + label, ft, zu._h, f, n, capi._np_ptr(i32(0, 0)))
        raw("follow_tracks.raw.stop " + label, ft, zu._h, f, n, NULL)
    raw("follow_tracks.raw.slot=-2", ft, zu._h, 0, 1, capi._np_ptr(i32(-2)))
    raw("follow_tracks.raw.slot=64", ft, zu._h, 0, 2, capi._np_ptr(i32(0, 64)))
    raw("follow_tracks.raw.slot=2^31-1", ft, zu._h, 0, 1, capi._np_ptr(i32(2 ** 31 - 1)))
    wrapped("follow_tracks.capi.slot=-2", zu.follow_tracks, [-2])
    wrapped("follow_tracks.capi.slot=64", zu.follow_tracks, [64])
    wrapped("follow_tracks.capi.first=4", zu.follow_tracks, [0], first=NCH)
    for k in ("s16", "s8", "frac"):
        raw("follow_tracks.raw.%s" % k, ft, objs[k]._h, 0, 1, capi._np_ptr(i32(0)))
        raw("follow_tracks.raw.%s and slot[1]=64" % k, ft, objs[k]._h, 0, 2, capi._np_ptr(i32(0, 64)))
        raw("follow_tracks.raw.%s and slot[0]=64" % k, ft, objs[k]._h, 0, 2, capi._np_ptr(i32(64, 0)))
        raw("follow_tracks.raw.%s and first=4" % k, ft, objs[k]._h, NCH, 1, capi._np_ptr(i32(0)))
        wrapped("follow_tracks.capi.%s" % k, objs[k].follow_tracks, [0])
    # a channel of another kind, in both directions: channel 1 follows its gain, 2 its scanner, 3 slot 5
    zu.follow_gain(True, 1, 1)
    zu.follow_scanner(True, 2, 1)
    zu.follow_tracks([5], first=3)
    for name, fn, meth, own in (("follow_scanner", fs, zu.follow_scanner, 2), ("follow_gain", fg, zu.follow_gain, 1)):
        for c, kind in ((1, "gain"), (2, "scanner"), (3, "track")):
            if c != own:
                raw("%s.raw.a %s follower" % (name, kind), fn, zu._h, c, 1, 1)
                wrapped("%s.capi.a %s follower" % (name, kind), meth, True, c, 1)
        raw("%s.raw.every channel" % name, fn, zu._h, 0, NCH, 1)              # the first obstacle in channel order
    raw("follow_scanner.raw.channels 3 and up", fs, zu._h, 3, 1, 1)
    raw("follow_gain.raw.channels 2 and up", fg, zu._h, 2, 2, 1)
    raw("follow_scanner.raw.channels 1 and up", fs, zu._h, 1, 3, 1)
    raw("follow_tracks.raw.a gain follower", ft, zu._h, 1, 1, capi._np_ptr(i32(0)))
    raw("follow_tracks.raw.a scanner follower", ft, zu._h, 2, 1, capi._np_ptr(i32(0)))
    raw("follow_tracks.raw.gain then scanner follower", ft, zu._h, 1, 2, capi._np_ptr(i32(0, 0)))
    raw("follow_tracks.raw.every channel", ft, zu._h, 0, NCH, capi._np_ptr(i32(0, 1, 2, 3)))
    raw("follow_tracks.raw.a scanner follower and slot[1]=64", ft, zu._h, 2, 2, capi._np_ptr(i32(0, 64)))
    wrapped("follow_tracks.capi.a gain follower", zu.follow_tracks, [0], first=1)
    wrapped("follow_tracks.capi.a scanner follower", zu.follow_tracks, [0], first=2)
    zu.follow_gain(False)
    zu.follow_scanner(False)
    zu.follow_tracks(None)

    stt = L.iqd_channelizer_set_track_table
    tgood = dict(slots_dev=dp["slots"], n_slots=8, n_blocks=1, block_bytes=64, lag=0, min_state=2, reserved=(0, 0, 0))

    def follow(**kw):
        v = dict(tgood, **kw)
        return capi.TrackFollow(v["slots_dev"] or None, v["n_slots"], v["n_blocks"], v["block_bytes"], v["lag"], v["min_state"],
                                (C.c_uint32 * 3)(*v["reserved"]))

    raw("set_track_table.raw.object NULL", stt, NULL, C.byref(follow()), untouched=True)
    TABLES = (("reserved[0]", dict(reserved=(1, 0, 0))), ("reserved[1]", dict(reserved=(0, 1, 0))), ("reserved[2]", dict(reserved=(0, 0, 1))),
              ("n_slots=0", dict(n_slots=0)), ("n_slots=65", dict(n_slots=65)), ("n_blocks=0", dict(n_blocks=0)), ("block_bytes=0", dict(block_bytes=0)),
              ("block_bytes=96", dict(block_bytes=96)), ("lag=2", dict(lag=2)), ("min_state=0", dict(min_state=0)), ("min_state=3", dict(min_state=3)),
              ("slots_dev NULL", dict(slots_dev=0)), ("slots_dev + 4", dict(slots_dev=dp["slots"] + 4)), ("slots_dev + 8", dict(slots_dev=dp["slots"] + 8)),
              ("reserved[2] and n_slots=0", dict(reserved=(0, 0, 1), n_slots=0)), ("n_slots=65 and n_blocks=0", dict(n_slots=65, n_blocks=0)),
              ("n_blocks=0 and block_bytes=96", dict(n_blocks=0, block_bytes=96)), ("block_bytes=96 and lag=2", dict(block_bytes=96, lag=2)),
              ("lag=2 and min_state=3", dict(lag=2, min_state=3)), ("min_state=3 and slots_dev NULL", dict(min_state=3, slots_dev=0)))
    for label, kw in TABLES:
        raw("set_track_table.raw." + label, stt, zu._h, C.byref(follow(**kw)))
        wrapped("set_track_table.capi." + label, zu.set_track_table, **dict(tgood, **kw))

    # ---- run and run_device ---------------------------------------------------------------------------------------------------
    run, rund = L.iqd_channelizer_run, L.iqd_channelizer_run_device

    def run_cases(z, tag, bps, lengths):
        """one object's refusals in both forms: p maps wide / out to pointers"""
        for form, fn, p, meth in (("run", run, hp, None), ("run_device", rund, dp, z.run_device)):
            name = "%s.raw.%s." % (form, tag)
            raw(name + "wide NULL", fn, z._h, NULL, bps, p["out"])
            raw(name + "out NULL", fn, z._h, p["wide"], bps, NULL)
            raw(name + "wide and out NULL", fn, z._h, NULL, bps, NULL)
            raw(name + "wide NULL and bytes=0", fn, z._h, NULL, 0, p["out"])
            for label, n in lengths:
                raw(name + label, fn, z._h, p["wide"], n, p["out"])
                if meth:
                    wrapped("%s.capi.%s.%s" % (form, tag, label), meth, p["wide"], n, p["out"])
        name = "run_device.raw.%s." % tag
        raw(name + "wide_dev + 4", rund, z._h, dp["wide"] + 4, bps, dp["out"])
        raw(name + "out_dev + 4", rund, z._h, dp["wide"], bps, dp["out"] + 4)
        raw(name + "out_dev + 8", rund, z._h, dp["wide"], bps, dp["out"] + 8)
        raw(name + "wide_dev + 4 and out NULL", rund, z._h, dp["wide"] + 4, bps, NULL)
        raw(name + "wide_dev + 4 and bytes=0", rund, z._h, dp["wide"] + 4, 0, dp["out"])
        wrapped("run_device.capi.%s.wide_dev + 4" % tag, z.run_device, dp["wide"] + 4, bps, dp["out"])
        wrapped("run_device.capi.%s.wide NULL" % tag, z.run_device, 0, bps, dp["out"])

    raw("run.raw.object NULL", run, NULL, hp["wide"], BPS, hp["out"], untouched=True)
    raw("run_device.raw.object NULL", rund, NULL, dp["wide"], BPS, dp["out"], untouched=True)
    LENGTHS = (("bytes=0", 0), ("bytes=448", BPS - 64), ("bytes=576", BPS + 64), ("bytes=2^31", 2 ** 31), ("bytes=2^32", 2 ** 32), ("bytes=2^38", 2 ** 38))
    run_cases(zu, "u8", BPS, LENGTHS)
    run_cases(z8, "s8", BPS, LENGTHS[:2] + LENGTHS[-1:])
    run_cases(z16, "s16", 2 * BPS, (("bytes=0", 0), ("bytes=512", BPS), ("bytes=1536", 3 * BPS), ("bytes=2^38", 2 ** 38)))
    run_cases(zf, "frac", FBPS, (("bytes=0", 0), ("bytes=512", BPS), ("bytes=4736", FBPS - 64), ("bytes=2^38", 2 ** 38),
                                 ("bytes=4800 * 2^19", FBPS << 19), ("bytes=4800 * 2^22", FBPS << 22)))
    wrapped("run.capi.u8.bytes=0", zu.run, np.zeros((SRC, 0), np.uint8))
    wrapped("run.capi.u8.bytes=448", zu.run, np.zeros((SRC, BPS - 64), np.uint8))
    wrapped("run.capi.s16.bytes=512", z16.run, np.zeros((SRC, BPS // 2), "<i2"))
    wrapped("run.capi.frac.bytes=512", zf.run, np.zeros((SRC, BPS), np.uint8))

    def with_follower(kind, tag, cases):
        """channel 2 of the U8 object follows (kind: scanner, gain, both), the cases run, it stops"""
        if kind in ("scanner", "both"):
            zu.follow_scanner(True, 2, 1)
        if kind in ("gain", "both"):
            zu.follow_gain(True, 1, 1)
        cases(tag)
        zu.follow_scanner(False)
        zu.follow_gain(False)

    def run_follower_cases(tag):
        for form, fn, p in (("run", run, hp), ("run_device", rund, dp)):
            name = "%s.raw.%s." % (form, tag)
            raw(name + "valid otherwise", fn, zu._h, p["wide"], BPS, p["out"])
            raw(name + "wide NULL", fn, zu._h, NULL, BPS, p["out"])
            raw(name + "bytes=448", fn, zu._h, p["wide"], BPS - 64, p["out"])
            raw(name + "bytes=0", fn, zu._h, p["wide"], 0, p["out"])
        raw("run_device.raw.%s.out_dev + 4" % tag, rund, zu._h, dp["wide"], BPS, dp["out"] + 4)
        wrapped("run_device.capi.%s.valid otherwise" % tag, zu.run_device, dp["wide"], BPS, dp["out"])
        wrapped("run.capi.%s.valid otherwise" % tag, zu.run, first["u8"])

    for kind in ("scanner", "gain", "both"):
        with_follower(kind, "a %s follower" % kind if kind != "both" else "a scanner and a gain follower", run_follower_cases)

    # the three track refusals, in every call form: no table, a slot the table does not have, the length rule
    acc, accd = L.iqd_accept_wideband, L.iqd_accept_wideband_device

    def call_forms(z, e, bps, first_ch=0):
        return (("run", lambda: run(z._h, hp["wide"], bps, hp["out"]), lambda: z.run(np.zeros((SRC, bps), np.uint8)) if bps < ROOM else None),
                ("run_device", lambda: rund(z._h, dp["wide"], bps, dp["out"]), lambda: z.run_device(dp["wide"], bps, dp["out"])),
                ("accept_wideband", lambda: acc(e._h, z._h, first_ch, hp["wide"], bps, hp["pcm"], hp["cnt"], hp["mag"], hp["sp"]),
                 lambda: e.accept_wideband(z, np.zeros((SRC, bps), np.uint8), first_ch) if bps < ROOM else None),
                ("accept_wideband_device", lambda: accd(e._h, z._h, first_ch, dp["wide"], bps, dp["out"], dp["pcm"], dp["cnt"], dp["mag"], dp["sp"]),
                 lambda: e.accept_wideband_device(z, dp["wide"], bps, dp["out"], dp["pcm"], dp["cnt"], dp["mag"], dp["sp"], first_ch)))

    def every_form(label, z, e, bps, first_ch=0, forms=None):
        for form, r, w in call_forms(z, e, bps, first_ch):
            if forms is None or form in forms:
                raw("%s.raw.%s" % (form, label), r)
                if bps and bps < ROOM:
                    wrapped("%s.capi.%s" % (form, label), w)

    zu.follow_tracks([5], first=3)
    every_form("track.no table", zu, eng, BPS)
    every_form("track.no table and bytes=448", zu, eng, BPS - 64)
    zu.set_track_table(**dict(tgood, n_slots=5))
    every_form("track.slot 5 of 5", zu, eng, BPS)
    every_form("track.slot 5 of 5 and bytes=0", zu, eng, 0)
    zu.set_track_table(**dict(tgood, n_blocks=2))
    every_form("track.two blocks of 64 for a row of 64", zu, eng, BPS)
    every_form("track.the length rule and bytes=448", zu, eng, BPS - 64)
    every_form("track.the length rule and first_ch=1", zu, eng, BPS, first_ch=1, forms=("accept_wideband", "accept_wideband_device"))
    zu.set_track_table(**dict(tgood, n_slots=5, n_blocks=2))
    every_form("track.slot 5 of 5 and the length rule", zu, eng, BPS)
    raw("run_device.raw.track.no table and wide_dev + 4", rund, zu._h, dp["wide"] + 4, BPS, dp["out"])
    raw("run.raw.track.slot 5 of 5 and out NULL", run, zu._h, hp["wide"], BPS, NULL)

    # ---- survey and survey_device -----------------------------------------------------------------------------------------------
    sv, svd = L.iqd_channelizer_survey, L.iqd_channelizer_survey_device

    def survey_forms(label, z, bps, block, capi_too=True):
        raw("survey.raw." + label, sv, z._h, hp["wide"], bps, block, hp["mag"])
        raw("survey_device.raw." + label, svd, z._h, dp["wide"], bps, block, dp["mag"])
        if capi_too:
            wrapped("survey_device.capi." + label, z.survey_device, dp["wide"], bps, block, dp["mag"])
            if bps < ROOM:
                wrapped("survey.capi." + label, z.survey, np.zeros((SRC, bps), np.uint8), block)

    raw("survey.raw.object NULL", sv, NULL, hp["wide"], BPS, 64, hp["mag"], untouched=True)
    raw("survey_device.raw.object NULL", svd, NULL, dp["wide"], BPS, 64, dp["mag"], untouched=True)
    survey_forms("no points and a track follower", zu, BPS, 64)
    zu.follow_tracks(None)
    survey_forms("no points", zu, BPS, 64)
    zu.follow_tracks([5], first=3)
    survey_forms("no points and bytes=0", zu, 0, 64, capi_too=False)
    survey_forms("frac.no points", zf, FBPS, 256)
    zu.set_survey(phase_inc=[0, 1 << 30])
    zf.set_survey(phase_inc=[0, 1 << 30])
    survey_forms("a track follower", zu, BPS, 64)
    survey_forms("a track follower and bytes=448", zu, BPS - 64, 64)
    zu.follow_tracks(None)
    zu.set_track_table(None)
    for kind in ("scanner", "gain", "both"):
        tag = "a %s follower" % kind if kind != "both" else "a scanner and a gain follower"
        with_follower(kind, tag, lambda t: (survey_forms(t, zu, BPS, 64), survey_forms(t + " and block_bytes=0", zu, BPS, 0)))
    zu.follow_scanner(True, 2, 1)
    zu.follow_tracks([5], first=3)
    survey_forms("a scanner and a track follower", zu, BPS, 64)
    zu.follow_scanner(False)
    zu.follow_tracks(None)
    for form, fn, p in (("survey", sv, hp), ("survey_device", svd, dp)):
        raw(form + ".raw.wide NULL", fn, zu._h, NULL, BPS, 64, p["mag"])
        raw(form + ".raw.magnitude NULL", fn, zu._h, p["wide"], BPS, 64, NULL)
        raw(form + ".raw.wide NULL and block_bytes=0", fn, zu._h, NULL, BPS, 0, p["mag"])
        raw(form + ".raw.magnitude NULL and bytes=0", fn, zu._h, p["wide"], 0, 64, NULL)
    raw("survey_device.raw.wide_dev + 4", svd, zu._h, dp["wide"] + 4, BPS, 64, dp["mag"])
    raw("survey_device.raw.magnitude_dev + 4", svd, zu._h, dp["wide"], BPS, 64, dp["mag"] + 4)
    raw("survey_device.raw.wide_dev + 4 and block_bytes=0", svd, zu._h, dp["wide"] + 4, BPS, 0, dp["mag"])
    raw("survey_device.raw.wide_dev + 4 and magnitude NULL", svd, zu._h, dp["wide"] + 4, BPS, 64, NULL)
    wrapped("survey_device.capi.magnitude_dev + 4", zu.survey_device, dp["wide"], BPS, 64, dp["mag"] + 4)
    wrapped("survey_device.capi.wide NULL", zu.survey_device, 0, BPS, 64, dp["mag"])
    for label, bps, block in (("bytes=0", 0, 64), ("bytes=448", BPS - 64, 64), ("bytes=2^38", 2 ** 38, 64), ("block_bytes=0", BPS, 0),
                              ("block_bytes=32", BPS, 32), ("block_bytes=96", 3 * BPS, 96), ("block_bytes=2^24+64", BPS, 2 ** 24 + 64),
                              ("block_bytes=2^32-64", BPS, 2 ** 32 - 64), ("block_bytes=128 on a row of 64", BPS, 128),
                              ("block_bytes=128 on a row of 192", 3 * BPS, 128), ("bytes=448 and block_bytes=0", BPS - 64, 0),
                              ("block_bytes=96 on a row of 64", BPS, 96)):
        survey_forms(label, zu, bps, block, capi_too=bps != 0)
    for label, bps, block in (("frac.block_bytes=64", FBPS, 64), ("frac.block_bytes=0", FBPS, 0), ("frac.block_bytes=2^24+256", FBPS, 2 ** 24 + 256),
                              ("frac.block_bytes=1024 on a row of 512", FBPS, 1024), ("frac.bytes=512", BPS, 256)):
        survey_forms(label, zf, bps, block)
    zu.set_survey(phase_inc=np.arange(4096, dtype=np.uint32) << 20)
    survey_forms("4096 points on 2^22 blocks", zu, 2 ** 31 - BPS, 64, capi_too=False)
    survey_forms("4096 points and block_bytes=128 on a row of 64", zu, BPS, 128)
    zu.set_survey(phase_inc=[])
    zf.set_survey(phase_inc=[])
    survey_forms("points cleared", zu, BPS, 64)

    # ---- accept_wideband and accept_wideband_device ---------------------------------------------------------------------------
    def accept(e, z, first_ch, p, bps, **kw):
        a = dict(p, **kw)
        if p is hp:
            return acc(e, z, first_ch, a["wide"], bps, a["pcm"], a["cnt"], a["mag"], a["sp"])
        return accd(e, z, first_ch, a["wide"], bps, a["out"], a["pcm"], a["cnt"], a["mag"], a["sp"])

    for form, p in (("accept_wideband", hp), ("accept_wideband_device", dp)):
        name = form + ".raw."
        raw(name + "engine NULL", accept, NULL, zu._h, 0, p, BPS, untouched=True)
        raw(name + "engine and object NULL", accept, NULL, NULL, 0, p, BPS, untouched=True)
        raw(name + "object NULL", accept, eng._h, NULL, 0, p, BPS)
        raw(name + "another engine's channelizer", accept, eng2._h, zu._h, 0, p, BPS, on=eng2)
        raw(name + "another engine's channelizer and wide NULL", accept, eng2._h, zu._h, 0, p, BPS, on=eng2, wide=NULL)
        raw(name + "another engine's channelizer and bytes=0", accept, eng._h, z_other._h, 0, p, 0)
        raw(name + "wide NULL", accept, eng._h, zu._h, 0, p, BPS, wide=NULL)
        raw(name + "pcm NULL", accept, eng._h, zu._h, 0, p, BPS, pcm=NULL)
        raw(name + "wide NULL and bytes=0", accept, eng._h, zu._h, 0, p, 0, wide=NULL)
        raw(name + "pcm NULL and first_ch=1", accept, eng._h, zu._h, 1, p, BPS, pcm=NULL)
        for label, n in LENGTHS:
            raw(name + label, accept, eng._h, zu._h, 0, p, n)
        raw(name + "s16.bytes=512", accept, eng._h, z16._h, 0, p, BPS)
        raw(name + "s8.bytes=0", accept, eng._h, z8._h, 0, p, 0)
        raw(name + "frac.bytes=512", accept, eng._h, zf._h, 0, p, BPS)
        raw(name + "first_ch=1", accept, eng._h, zu._h, 1, p, BPS)
        raw(name + "first_ch=4", accept, eng._h, zu._h, NCH, p, BPS)
        raw(name + "first_ch=2^32-1", accept, eng._h, zu._h, 2 ** 32 - 1, p, BPS)
        raw(name + "four channels into an engine of two", accept, eng2._h, z_other._h, 0, p, BPS, on=eng2)
        raw(name + "a row of 320 in blocks of 256", accept, eng._h, zu._h, 0, p, 5 * BPS)
        raw(name + "s16.a row of 320 in blocks of 256", accept, eng._h, z16._h, 0, p, 10 * BPS)
        raw(name + "bytes=448 and first_ch=1", accept, eng._h, zu._h, 1, p, BPS - 64)
        raw(name + "bytes=2^38 and first_ch=4", accept, eng._h, zu._h, NCH, p, 2 ** 38)
        raw(name + "first_ch=1 and a row of 320", accept, eng._h, zu._h, 1, p, 5 * BPS)
    raw("accept_wideband_device.raw.rows NULL", accept, eng._h, zu._h, 0, dp, BPS, out=NULL)
    raw("accept_wideband_device.raw.wide_dev + 4", accept, eng._h, zu._h, 0, dp, BPS, wide=dp["wide"] + 4)
    raw("accept_wideband_device.raw.rows_dev + 4", accept, eng._h, zu._h, 0, dp, BPS, out=dp["out"] + 4)
    raw("accept_wideband_device.raw.rows_dev + 4 and pcm NULL", accept, eng._h, zu._h, 0, dp, BPS, out=dp["out"] + 4, pcm=NULL)
    raw("accept_wideband_device.raw.wide_dev + 4 and bytes=0", accept, eng._h, zu._h, 0, dp, 0, wide=dp["wide"] + 4)
    raw("accept_wideband_device.raw.wide_dev + 4 and first_ch=1", accept, eng._h, zu._h, 1, dp, BPS, wide=dp["wide"] + 4)
    raw("accept_wideband_device.raw.rows_dev + 4 on another engine", accept, eng2._h, zu._h, 0, dp, BPS, on=eng2, out=dp["out"] + 4)
    wrapped("accept_wideband.capi.another engine's channelizer", eng2.accept_wideband, zu, first["u8"])
    wrapped("accept_wideband.capi.bytes=448", eng.accept_wideband, zu, np.zeros((SRC, BPS - 64), np.uint8))
    wrapped("accept_wideband.capi.first_ch=1", eng.accept_wideband, zu, first["u8"], 1)
    wrapped("accept_wideband.capi.four channels into an engine of two", eng2.accept_wideband, z_other, first["u8"])
    wrapped("accept_wideband.capi.a row of 320 in blocks of 256", eng.accept_wideband, zu, np.zeros((SRC, 5 * BPS), np.uint8))
    wrapped("accept_wideband.capi.s16.bytes=512", eng.accept_wideband, z16, np.zeros((SRC, BPS // 2), "<i2"))
    wrapped("accept_wideband_device.capi.another engine's channelizer", eng2.accept_wideband_device, zu, dp["wide"], BPS, dp["out"], dp["pcm"])
    wrapped("accept_wideband_device.capi.wide_dev + 4", eng.accept_wideband_device, zu, dp["wide"] + 4, BPS, dp["out"], dp["pcm"])
    wrapped("accept_wideband_device.capi.pcm NULL", eng.accept_wideband_device, zu, dp["wide"], BPS, dp["out"], 0)
    wrapped("accept_wideband_device.capi.bytes=448", eng.accept_wideband_device, zu, dp["wide"], BPS - 64, dp["out"], dp["pcm"])
    wrapped("accept_wideband_device.capi.first_ch=1", eng.accept_wideband_device, zu, dp["wide"], BPS, dp["out"], dp["pcm"], first=1)
    wrapped("accept_wideband_device.capi.a row of 320 in blocks of 256", eng.accept_wideband_device, zu, dp["wide"], 5 * BPS, dp["out"], dp["pcm"])

    # ---- host-only functions ----------------------------------------------------------------------------------------------------
    inc = C.c_uint32()
    dt, dtq = L.iqd_channelizer_default_taps, L.iqd_channelizer_default_taps_q
    for label, fn, args in (
            ("phasor_table.out NULL", L.iqd_channelizer_phasor_table, (NULL,)),
            ("default_taps.decimation=1", dt, (1, NULL, 0)), ("default_taps.decimation=65", dt, (65, NULL, 0)),
            ("default_taps.out NULL with capacity", dt, (M, NULL, 4)),
            ("default_taps_q.den=3", dtq, (M, 3, NULL, 0)), ("default_taps_q.8/2", dtq, (8, 2, NULL, 0)), ("default_taps_q.15/8", dtq, (15, 8, NULL, 0)),
            ("default_taps_q.513/8", dtq, (513, 8, NULL, 0)), ("default_taps_q.out NULL with capacity", dtq, (FP, FQ, NULL, 4)),
            ("tuning.decimation=1", L.iqd_channelizer_tuning, (1, 100000000, 100000000, 0, C.byref(inc))),
            ("tuning.decimation=65", L.iqd_channelizer_tuning, (65, 100000000, 100000000, 0, C.byref(inc))),
            ("tuning.rotation=2", L.iqd_channelizer_tuning, (M, 100000000, 100000000, 2, C.byref(inc))),
            ("tuning.rotation=-2", L.iqd_channelizer_tuning, (M, 100000000, 100000000, -2, C.byref(inc))),
            ("tuning.inc NULL", L.iqd_channelizer_tuning, (M, 100000000, 100000000, 0, NULL)),
            ("tuning.out of band above", L.iqd_channelizer_tuning, (M, 100000000, 101024000, 0, C.byref(inc))),
            ("tuning.out of band below", L.iqd_channelizer_tuning, (M, 100000000, 98975999, 0, C.byref(inc))),
            ("window_outputs.decimation=1", L.iqd_channelizer_window_outputs, (1, 105, 0)),
            ("window_outputs.decimation=65", L.iqd_channelizer_window_outputs, (65, 105, 0)),
            ("window_outputs.n_taps=0", L.iqd_channelizer_window_outputs, (M, 0, 0)),
            ("window_outputs.n_taps=1025", L.iqd_channelizer_window_outputs, (M, 1025, 0)),
            ("window_outputs.sample_format=3", L.iqd_channelizer_window_outputs, (M, 105, 3)),
            ("track_window_outputs.decimation=1", L.iqd_channelizer_track_window_outputs, (1, 105)),
            ("track_window_outputs.decimation=65", L.iqd_channelizer_track_window_outputs, (65, 105)),
            ("track_window_outputs.n_taps=0", L.iqd_channelizer_track_window_outputs, (M, 0)),
            ("track_window_outputs.n_taps=1025", L.iqd_channelizer_track_window_outputs, (M, 1025))):
        raw("host." + label, fn, *args, untouched=True)
    wrapped("host.capi.default_taps.decimation=65", capi.channelizer_default_taps, 65)
    wrapped("host.capi.default_taps.8/2", capi.channelizer_default_taps, 8, 2)

    # ---- the second valid run of every object -----------------------------------------------------------------------------------
    eng.synchronize()
    for k, z in objs.items():
        rows[k].append(z.run(second[k]))
    for p in dp.values():
        eng.dev_free(p)
    for z in list(objs.values()) + [z_other]:
        z.close()
    eng.close()
    eng2.close()
    return dict(table=table, rows={k: np.concatenate(v, axis=1) for k, v in rows.items()}, want=model(capi, first, second))


def dump(table):
    return json.dumps(table, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    from rtlsdrdiags_amd import capi as _capi
    got = collect(_capi)
    for k, r in got["rows"].items():
        assert np.array_equal(r, got["want"][k]), k
    with open(sys.argv[1], "w") as f:
        f.write(dump(got["table"]))
    print("%d refusals -> %s" % (len(got["table"]), sys.argv[1]))
