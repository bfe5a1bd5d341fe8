"""The inputs that make hand-offs fail on purpose, for the CPU tier (tests/test_handoff_model_host.py: the predictor qualifies
every case - which hand-offs are bad, and that this is what the case is for) and for the device (tests/test_gpu_repairs.py runs
exactly these rows and holds the counters to the prediction).

Why they fail: the square pattern 255,255,255,255,0,0,0,0 (period 4 samples) keeps two de-emphasis trajectories apart for ever,
so a piece that warms up from zero inside such a stretch does not land on the exact state; a noiseless carrier leaves the exact
state stuck at a denormal while a zero-state warm-up sits at exactly 0, which counts as agreeing only where the gain allows it
(WBFM: K >= 1, DC removal: |gain| <= 1e6).  Whether a stretch breaks a hand-off depends on the state it is entered with and on
where the boundaries lie, so every row is built FROM the planner's segment length and then qualified by the model.

A case is a list of calls on one engine; a call gives every channel a row of the same length.  `purpose[call][channel]` is
"none" or (what, the number of bad hand-offs):
  all        every hand-off is bad (but those whose warm-up starts at the stream's own zero start)
  then_good  a run of bad hand-offs from the first on, then good ones to the end
  then_bad   good hand-offs, then bad ones to the end
  isolated   single bad hand-offs, each with a good one before and after it
  last       only the hand-off into segment ntiles - 2, in front of a last segment shorter than FORCED_BACK
  none       no bad hand-off, and nothing for the first look to flag"""
import collections

import numpy as np

from rtlsdrdiags_amd import synth
from tests import emu_bind, handoff_model as H

GEOM = H.consts(emu_bind.lib())     # ST_HALO, COLD_HALO, FORCED_BACK, DC_TILE, DC_WARM: the kernels' own, through the emulation library

TILES, STREAM = 0x2, 0x4            # IQD_F_WBFM_TILES, IQD_F_WBFM_STREAM
PLAN_TILES, PLAN_STREAM = 0, 1
SQUARE = np.array([255, 255, 255, 255, 0, 0, 0, 0], np.uint8)
QUIET_THRESHOLD = -38               # closes on digital silence, open on everything else here
DC_GAIN_AGREES = np.float32(1e6)    # the largest gain at which two sub-2^-100 DC states count as agreeing
DC_GAIN_ABOVE = np.nextafter(np.float32(1e6), np.float32(2e6))


def square(n):
    return np.tile(SQUARE, n // 4)


def carrier(n, amp=60):
    """A noiseless carrier at -Fs/4: exactly constant after the front-end rotation."""
    pat = np.array([[amp, 0], [0, -amp], [-amp, 0], [0, amp]], np.int16)
    return (128 + np.tile(pat, (n // 4, 1))).astype(np.uint8).reshape(-1)


_FM = {}


def fm(n, seed):
    if (n, seed) not in _FM:
        _FM[(n, seed)] = synth.fm_tone(n, seed=seed)
    return _FM[(n, seed)].copy()


def with_square(n, stretches, seed):
    """FM with the square pattern over the sample ranges `stretches` (multiples of 4)"""
    u8 = fm(n, seed)
    for lo, hi in stretches:
        lo, hi = max(0, lo // 4 * 4), min(n, hi // 4 * 4)
        u8[2 * lo:2 * hi] = square(hi - lo)
    return u8


def punch(u8, block_bytes, at_blocks, extra=2):
    """Squelch-gated rows: virtual block b of `at_blocks` becomes digital silence and `extra` silent blocks follow it (the squelch
    still lets the first one through, then closes); the row keeps its length, so it loses its last extra * len(at_blocks)
    blocks.  The demodulator then sees u8 with those blocks silenced, cut short."""
    blocks = u8.reshape(-1, block_bytes)
    out = []
    for b in range(len(blocks)):
        if b in at_blocks:
            out.extend([np.full(block_bytes, 128, np.uint8)] * (1 + extra))
        else:
            out.append(blocks[b])
    return np.concatenate(out)[:len(u8)]


def stretch_for(form, b, tail=100):
    """The square stretch that breaks the hand-off at boundary b and no other: it begins 24 samples before the zero-state warm-up
    of the piece behind b does, so that the warm-up never sees the input the exact state came in on, and ends `tail` samples behind
    the point of comparison.  With a tail of 700 a streamed segment's inexact run stays an ulp off almost to its end, so the
    histories it hands to the segment behind it - whose own warm-up, begun 792 samples into the stretch, does land on the exact
    state - are inexact: the case for the `redo_next` rule of wbfm_repair_body (at a gain where an ulp reaches the sample).
    (Found with the model: a stretch that begins 200 samples earlier breaks nothing - the exact trajectory and the warm-up then
    settle on the same periodic orbit.)"""
    off = 0 if form == "stream" else GEOM["FORCED_BACK"]       # the tile kernel compares FORCED_BACK before the boundary ...
    lead = GEOM["ST_HALO"] if form == "stream" else GEOM["COLD_HALO"] - GEOM["FORCED_BACK"]   # ... after that many zero-state steps
    return (b - off - lead - 24, b - off + tail)


Case = collections.namedtuple("Case", "name kind form flags n_calls modes threshold block_bytes min_seg gains purpose build shape partner")
CASES = collections.OrderedDict()


def _add(name, kind, form, modes, purpose, build, n_calls=2, threshold=None, block_bytes=0, min_seg=0, gains=None, shape=None, partner=None):
    flags = {"tiles": TILES, "stream": STREAM, "mixed": 0, "dc": 0, "dc_stream": STREAM}[form]
    if kind == "wbfm":
        block_bytes = 256                   # (rows are whole blocks: 128-sample ones, so that the row lengths are free)
    CASES[name] = Case(name, kind, form, flags, n_calls, tuple(modes), threshold, block_bytes, min_seg, gains or {}, purpose, build, shape, partner)


# ---- WBFM: the four launch forms, each with the three failing inputs and a clean one, then a clean call ---------------------
N_FORM = 86 * 768                   # 66048 samples: 86 streamed segments (a full last one), 10 tiles of the tile kernel


def _form_rows(tile_len, form, n, gated_blocks=None):
    """Rows 'all', 'then_good', 'isolated', 'none' of one call for segments of tile_len samples."""
    nb = (n - 1) // tile_len                                   # boundaries
    i1, i2 = max(2, nb // 4), max(4, (2 * nb) // 3)
    rows = [square(n),
            with_square(n, [(0, tile_len * max(3, nb // 3) + tile_len // 2)], 11),
            with_square(n, [stretch_for(form, tile_len * i1), stretch_for(form, tile_len * i2, 700)], 12),
            with_square(n, [(20000, n)], 5)]
    if gated_blocks:
        rows = [punch(r, 256, blk) for r, blk in zip(rows, gated_blocks)]
    return rows


def _build_form(form, gated):
    def build(tile_len):
        # (silenced blocks away from the stretches that matter; a different number per channel, so that vlen_gated differs)
        blocks = [(2,), (300, 450), (5, 250, 480), ()] if gated else None
        first = np.stack(_form_rows(tile_len, form, N_FORM, blocks))
        clean = np.stack([fm(N_FORM, 20 + c) for c in range(4)])
        if gated:
            clean = np.stack([punch(r, 256, blk) for r, blk in zip(clean, [(100,), (), (7, 8, 200), (350,)])])
        return [first, clean]
    return build


# At the default gain an ulp of state error rarely reaches a sample: (int16)y of a state around 10^3 is the same for both.  At a
# demodulator gain of 5e8 (the casts stay bounded: K * 3.173 = 6.9e8 < 2^31) the state is around 2^24 and beyond, where an ulp is
# units of the integer cast, whose low 16 bits are the sample: every inexact state shows in the PCM.  (Worked out on the CPU
# with the oracle's decimators: histories taken from a segment's inexact run change the first 17 PCM samples of the segment
# behind it at 5e8 and at 2e8, none at 5e7 or below - there the +-1 differences round away in the three Q15 decimators.)
# Each form runs at both gains.
LOUD_GAIN = 5.0e8

for _form in ("tiles", "stream"):
    for _gated in (False, True):
        for _loud in (False, True):
            _add("wbfm_%s%s%s" % (_form, "_gated" if _gated else "", "_loud" if _loud else ""), "wbfm", _form, ["wbfm"] * 4,
                 [[("all", 9 if _form == "tiles" else 84), ("then_good", 3 if _form == "tiles" else 27), ("isolated", 2), "none"],
                  ["none"] * 4], _build_form(_form, _gated),
                 threshold=QUIET_THRESHOLD if _gated else None, gains={c: ("wbfm", LOUD_GAIN) for c in range(4)} if _loud else None)

# ---- a short last segment: the keeper rule (wbfm_repair_body, wbfm_pick_carry) ------------------------------------------------
N_SHORT = 1 << 16                   # 85 segments of 768 samples and a last one of 256


def _build_short(tile_len):
    nb = (N_SHORT - 1) // tile_len
    b = tile_len * (nb - 1)                                    # the hand-off into segment ntiles - 2
    first = np.stack([with_square(N_SHORT, [stretch_for("stream", b)], 31), square(N_SHORT), fm(N_SHORT, 32)])
    return [first, np.stack([fm(N_SHORT, 33 + c) for c in range(3)])]


for _ms in (0, 1):
    for _loud in (False, True):
        _add("wbfm_short_last" + ("_min_seg_1" if _ms else "") + ("_loud" if _loud else ""), "wbfm", "stream", ["wbfm"] * 3,
             [[("last", 1), ("all", 84), "none"], ["none"] * 3], _build_short, min_seg=_ms,
             gains={c: ("wbfm", LOUD_GAIN) for c in range(3)} if _loud else None)

# ---- repaired calls in a row over one stream (fed to a streaming and a tile-kernel engine alike) -----------------------------
N_ROW = 43 * 768


def _build_in_a_row(tile_lens):
    """the same four rows for both kernels (tile_lens: the segment length of either): the third call has a stretch for either
    kernel's segments, at the middle boundary"""
    n = N_ROW
    both = [stretch_for(form, T * (((n - 1) // T) // 2)) for form, T in sorted(tile_lens.items())]
    return [square(n)[None], with_square(n, [(0, 2 * n // 3)], 41)[None], with_square(n, both, 42)[None], fm(n, 43)[None]]


_add("wbfm_in_a_row_stream", "wbfm", "stream", ["wbfm"], [[("all", 41)], [("then_good", 28)], [("isolated", 2)], ["none"]],
     _build_in_a_row, n_calls=4, partner="wbfm_in_a_row_tiles")
_add("wbfm_in_a_row_tiles", "wbfm", "tiles", ["wbfm"], [[("all", 4)], [("then_good", 3)], [("isolated", 1)], ["none"]],
     _build_in_a_row, n_calls=4, partner="wbfm_in_a_row_stream")

# ---- K < 1: the sub-2^-100 exception must not apply ------------------------------------------------------------------------------
# A modulated stretch, then the noiseless carrier for the rest of the call and all of the next one: the exact state decays into
# the denormals and sticks there, a zero-state warm-up sits at exactly 0.  At the default gain (K >= 1) every hand-off of the
# second call agrees by the exception; at gain 1.0 (K < 1) every one is bad.  In the FIRST call a hand-off is bad at either gain
# when its warm-up begins behind the stretch (or too few samples before its end to converge) and it is compared less than some
# 1460 samples behind it: the exact state there is still decaying (1e3 x 0.949^n > 2^-100), no exception covers that.  Streamed
# segments warm up over 768 samples and are compared every 768, so one of them always meets it, wherever the stretch ends - the
# 0 at the default gain is therefore asserted on the second call; the tile kernel's first call is clean at the default gain.
def _build_k(tile_len):
    return [np.concatenate([fm(8192, 51), carrier(N_FORM - 8192)])[None], carrier(N_FORM)[None], fm(N_FORM, 52)[None]]


for _form in ("stream", "tiles"):
    _nb = 85 if _form == "stream" else 9
    _add("wbfm_k_below_1_" + _form, "wbfm", _form, ["wbfm"], [[("then_bad", 74 if _form == "stream" else 8)], [("all", _nb)], ["none"]],
         _build_k, n_calls=3, gains={0: ("wbfm", 1.0)})
    _add("wbfm_k_default_" + _form, "wbfm", _form, ["wbfm"], [[("isolated", 1) if _form == "stream" else "none"], ["none"], ["none"]], _build_k, n_calls=3)

# ---- DC removal (AM and one SSB sideband): rows of more than one DC tile -------------------------------------------------------
N_DC2, N_DC3 = 2 * GEOM["DC_TILE"] * 32 + 16384, 3 * GEOM["DC_TILE"] * 32 + 65536   # just over two and three DC tiles, whole 16384-sample blocks


def decaying(n, mode, seed, stop=GEOM["DC_TILE"] - GEOM["DC_WARM"] - 600):
    """modulated up to 8 kS/s sample `stop`, then the noiseless carrier: the detector's output becomes constant"""
    u8 = (synth.am_tone(n, seed=seed, tone=700.0, depth=0.8) if mode == "am" else synth.ssb_tone(n, seed=seed)).copy()
    u8[64 * stop:] = carrier(n - 32 * stop)
    return u8


def live(n, mode, seed):
    return synth.am_tone(n, seed=seed, tone=440.0, depth=0.6) if mode == "am" else synth.ssb_tone(n, seed=seed)


def _build_dc(mode, n, n_ch=1, blocks=None):
    def build(_):
        first = [decaying(n, mode, 61) if n_ch == 1 or c == 1 else live(n, mode, 62 + c) for c in range(n_ch)]
        second = [live(n, mode, 70 + c) for c in range(n_ch)]
        if blocks:
            first = [punch(r, 32768, blocks) for r in first]
            second = [punch(r, 32768, (3,)) for r in second]
        return [np.stack(first), np.stack(second)]
    return build


for _mode in ("am", "usb"):
    _fam = "am" if _mode == "am" else "ssb"
    _add("dc_%s_at_1e6" % _mode, "dc", "dc", [_mode], [["none"], ["none"]], _build_dc(_mode, N_DC2), gains={0: (_fam, DC_GAIN_AGREES)})
    _add("dc_%s_above_1e6" % _mode, "dc", "dc", [_mode], [[("all", 2)], ["none"]], _build_dc(_mode, N_DC2), gains={0: (_fam, DC_GAIN_ABOVE)})
    _add("dc_%s_gated_at_1e6" % _mode, "dc", "dc", [_mode], [["none"], ["none"]], _build_dc(_mode, N_DC3, blocks=(1,)),
         threshold=QUIET_THRESHOLD, block_bytes=32768, gains={0: (_fam, DC_GAIN_AGREES)})
    _add("dc_%s_gated_above_1e6" % _mode, "dc", "dc", [_mode], [[("all", 3)], ["none"]], _build_dc(_mode, N_DC3, blocks=(1,)),
         threshold=QUIET_THRESHOLD, block_bytes=32768, gains={0: (_fam, DC_GAIN_ABOVE)})
_add("dc_am_middle_of_three", "dc", "dc", ["am"] * 3, [["none", ("all", 2), "none"], ["none"] * 3], _build_dc("am", N_DC2, n_ch=3),
     gains={c: ("am", DC_GAIN_ABOVE) for c in range(3)})

# ---- a periodic detector stream that keeps two DC trajectories apart at the DEFAULT gain: found by a search over noiseless
# square envelopes of period 2 .. 16 PCM samples, AM and USB (PERIODIC_FAMILY; tests/test_handoff_model_host.py runs the search and
# pins how many of them break a hand-off of a two-tile row); these two break both hand-offs, with PCM far from zero -------------
PERIODIC_FAMILY = [(mode, period, 60) for mode in ("am", "usb") for period in range(2, 17)]
PERIODIC_CHOSEN = [("am", 3, 60), ("usb", 14, 60)]



def periodic(n, mode, period, amp):
    t = np.arange(n)
    ph = (t % (32 * period)) / (32.0 * period)
    z = amp * np.where(ph < 0.5, 1.0, 0.3) * np.exp(-0.5j * np.pi * t)
    if mode != "am":
        z = z * np.exp(2j * np.pi * ph)                         # a tone at the envelope's period
    u8 = np.empty(2 * n, np.uint8)
    u8[0::2] = np.clip(np.rint(z.real) + 128, 0, 255)
    u8[1::2] = np.clip(np.rint(z.imag) + 128, 0, 255)
    return u8


def _build_periodic(mode, period):
    def build(_):
        assert (mode, period, 60) in PERIODIC_CHOSEN
        return [periodic(N_DC2, mode, period, 60)[None], live(N_DC2, mode, 75)[None]]
    return build


_add("dc_am_periodic", "dc", "dc", ["am"], [[("all", 2)], ["none"]], _build_periodic("am", 3))
_add("dc_usb_periodic", "dc", "dc", ["usb"], [[("all", 2)], ["none"]], _build_periodic("usb", 14))
# ... and at a gain of 1e6, where gain * y is around 2^24 and an ulp of y is a unit of the cast: a tile left unrepaired shows in the PCM
_add("dc_am_periodic_loud", "dc", "dc", ["am"], [[("all", 2)], ["none"]], _build_periodic("am", 3), gains={0: ("am", DC_GAIN_AGREES)})
_add("dc_usb_periodic_loud", "dc", "dc", ["usb"], [[("all", 2)], ["none"]], _build_periodic("usb", 14), gains={0: ("ssb", DC_GAIN_AGREES)})

# ---- the `again` loop of dc_block_wave: one DC tile, streamed, in place over the int16 detector values --------------------------
N_AGAIN = 4096 * 32                 # two passes of the wave


def _build_again(_):
    return [decaying(N_AGAIN, "am", 81, stop=700)[None], live(N_AGAIN, "am", 82)[None]]


_add("dc_again_loop", "dc", "dc_stream", ["am"], [["none"], ["none"]], _build_again, gains={0: ("am", DC_GAIN_ABOVE)})


# ---- the one-launch mixed kernel: a shape of tests/one_launch_shapes.py, WBFM channels with failing rows beside clean ones,
# AM / FM / SSB families beside them ---------------------------------------------------------------------------------------------
MIXED_SHAPE = "mix"                 # 20 AM + 20 FM + 20 WBFM + 40 SSB x 2^14: 22 segments of 768 samples, the last one 256


def mixed_layout():
    import one_launch_shapes as S
    left, out = dict(S.SHAPES[MIXED_SHAPE].counts), []
    k = dict.fromkeys(S.FAMS, 0)
    while any(left.values()):
        for f in ("am", "fm", "wbfm", "ssb", "ssb"):
            if left[f]:
                out.append((f if f != "ssb" else ("lsb", "usb")[k[f] % 2], 1 if f == "wbfm" else S.SELECTORS[k[f] % 3]))
                left[f] -= 1
                k[f] += 1
    return out


MIXED_PURPOSES = (("all", 20), ("then_good", 5), ("isolated", 2), "none", ("last", 1))


def _build_mixed(tile_len):
    import one_launch_shapes as S
    n = S.SHAPES[MIXED_SHAPE].n
    nb = (n - 1) // tile_len
    first, second, w = [], [], 0
    for c, (mode, _) in enumerate(mixed_layout()):
        if mode == "wbfm":
            first.append([square(n), with_square(n, [(0, 6 * tile_len + 300)], 90 + w),
                          with_square(n, [stretch_for("stream", 5 * tile_len), stretch_for("stream", 13 * tile_len, 700)], 90 + w),
                          fm(n, 90 + w), with_square(n, [stretch_for("stream", (nb - 1) * tile_len)], 90 + w)][w % 5])
            w += 1
        else:
            first.append(np.roll(fm(n, 100 + c % 7), 2 * ((c * 37) % 1009)))
        second.append(np.roll(fm(n, 110 + c % 7), 2 * ((c * 53) % 1013)))
    return [np.stack(first), np.stack(second)]


_m = mixed_layout()
_add("mixed_one_launch", "mixed", "mixed", [m for m, _ in _m],
     [["none" if m != "wbfm" else MIXED_PURPOSES[[x for x, _ in _m[:c]].count("wbfm") % 5] for c, (m, _) in enumerate(_m)],
      ["none"] * len(_m)], _build_mixed, shape=MIXED_SHAPE)


# ---- the plan and the prediction -------------------------------------------------------------------------------------------------
def family_of(mode):
    return mode if mode in ("am", "fm", "wbfm") else "ssb"


def plan_of(case, plan_call, n):
    """Holds the case's call of n samples to the planner: the launch form it is for.  Returns the WBFM segment length (or the DC
    tile for the DC cases)."""
    gated = case.threshold is not None
    if case.kind == "mixed":
        import one_launch_shapes as S
        p, _ = S.hold(plan_call, S.SHAPES[case.shape])
        return p["fam"]["wbfm"]["tile_len"]
    if case.kind == "wbfm":
        p = plan_call(n, {"wbfm": ((len(case.modes), 0, 0), True, False)}, flags=case.flags, gated=gated, min_seg=case.min_seg)
        q = p["fam"]["wbfm"]
        want = PLAN_STREAM if case.form == "stream" else PLAN_TILES
        assert q["path"] == want and not p["fused"], (case.name, "the planner has moved", q)
        assert q["tiles_per_ch"] >= 3, (case.name, q)
        return q["tile_len"]
    fam = family_of(case.modes[0])
    p = plan_call(n, {fam: ((len(case.modes), 0, 0), True, False)}, flags=case.flags, gated=gated)
    q = p["fam"][fam]
    assert q["path"] == (PLAN_STREAM if case.form == "dc_stream" else PLAN_TILES), (case.name, "the planner has moved", q)
    return GEOM["DC_TILE"]


def qualify(case, oracle, L, plan_call):
    """The case's rows, built from the segment length the planner gives for their length, every call held to the planner
    (plan_of asserts the launch form the case is for), and the prediction per call."""
    def lens(n):
        if not case.partner:
            return plan_of(case, plan_call, n)
        return {c.form: plan_of(c, plan_call, n) for c in (case, CASES[case.partner])}
    n = 1 << 16
    for _ in range(2):                                        # (the planner wants the row length, the rows want its answer)
        rows = case.build(lens(n))
        n = rows[0].shape[1] // 2
    tile_lens = [plan_of(case, plan_call, r.shape[1] // 2) for r in rows]
    assert all(np.array_equal(a, b) for a, b in zip(rows, case.build(lens(n))))
    return rows, predict(case, rows, oracle, L, tile_lens)


Prediction = collections.namedtuple("Prediction", "tile_len bounds bad flagged handoffs vlen plain")


def predict(case, rows, oracle, L, tile_lens):
    """Per call: per channel the boundaries (in the channel's own stream of open samples), the bad hand-offs, what the first
    look flags and (WBFM) what the plain rule - a lead-in of ST_HALO / COLD_HALO samples ending AT the boundary - calls bad; and the
    number of hand-offs of the call."""
    n_ch = len(case.modes)
    streams, models = [], []
    for c in range(n_ch):
        if case.threshold is None:
            streams.append([r[c] for r in rows])
        else:
            chain = H.squelch_chain(oracle, case.threshold)
            streams.append([H.open_samples(chain, r[c], case.block_bytes)[0] for r in rows])
        whole = np.concatenate(streams[c])
        gain = case.gains.get(c, (None, None))[1]
        if case.modes[c] == "wbfm":
            models.append(H.Deemph(L, oracle, whole, gain=gain))
        elif case.kind != "dc":
            models.append(None)                              # (FM has no float state; AM / SSB rows of one DC tile have no boundary)
        else:
            models.append(H.DcRemoval(L, oracle, whole, case.modes[c], gain=300.0 if gain is None else gain))
    out, pos = [], [0] * n_ch
    for k in range(len(rows)):
        T = tile_lens[k]
        bounds, bad, flagged, plain, vlens = [], [], [], [], []
        for c in range(n_ch):
            vlen = len(streams[c][k]) // 2
            m = models[c]
            b, bd, fl, pl = [], [], [], []
            if m is not None and case.modes[c] == "wbfm":
                form = "tiles" if case.form == "tiles" else "stream"
                b = [pos[c] + T * i for i in range(1, (vlen + T - 1) // T)]
                bd, fl = m.bad(b, form), m.flagged(pos[c], b, form)
                pl = m.bad_by_the_plain_rule(b, GEOM["COLD_HALO"] if form == "tiles" else GEOM["ST_HALO"])
            elif m is not None:
                n8, p8 = vlen // 32, pos[c] // 32
                b = m.bounds(p8, n8) if rows[k].shape[1] // 64 > GEOM["DC_TILE"] else []   # (a row of one DC tile takes the one-wave pass)
                bd, fl = m.bad(b), m.flagged(p8, b)
            for lst, v in ((bounds, b), (bad, bd), (flagged, fl), (plain, pl), (vlens, vlen)):
                lst.append(v)
            pos[c] += vlen
        out.append(Prediction(T, bounds, bad, flagged, sum(len(b) for b in bounds), vlens, plain))
    return out


def purpose_holds(purpose, bounds, bad, flagged, first_call):
    """Is the predicted set of bad hand-offs what the row is for?"""
    if purpose == "none":
        return not bad and not flagged
    what, count = purpose
    bad_set = set(bad)
    idx = [i for i, b in enumerate(bounds) if b in bad_set]
    nb = len(bounds)
    if len(idx) != count or not idx or not flagged:
        return False
    if what == "all":
        return idx == list(range(1 if first_call else 0, nb)) or idx == list(range(nb))
    if what == "then_good":
        return idx == list(range(idx[0], idx[-1] + 1)) and idx[0] <= 1 and idx[-1] <= nb - 2
    if what == "then_bad":
        return idx == list(range(idx[0], nb)) and idx[0] >= 1
    if what == "isolated":
        return idx[0] >= 1 and idx[-1] <= nb - 2 and all(j - i > 1 for i, j in zip(idx, idx[1:]))
    if what == "last":
        return idx == [nb - 2]
    raise ValueError(purpose)
