"""CPU predictor of the hand-offs that do NOT chain up - the ones the device has to repair (tests/test_handoff_model_host.py
qualifies every case of tests/repair_cases.py with it, tests/test_gpu_repairs.py holds the device to what it predicts).

Two float recurrences cross segment boundaries, and both start their interior pieces from the zero state:

  de-emphasis   y = (u + u_prev) - a1 * y      IQD_IIR_STEP (iqd_wbfm.h), u[n] = b0 * (K * dtheta[n])
      a streamed segment warms up over the ST_HALO = 768 samples before its start and is checked AT its start against its
      predecessor's end state (iqd_stream_fix.h); a tile of the tile kernel warms up over COLD_HALO = 2048 samples and is checked
      FORCED_BACK = 768 samples before its start - after COLD_HALO - FORCED_BACK = 1280 steps - against the restart record its
      predecessor took there (wbfm_tile: rec.y_in, wbfm_verify_kernel);
  DC removal    y = (x - x_prev) - a1 * y      dc_block_run (iqd_chains.h) over the 8 kS/s detector stream
      tile k >= 1 of DC_TILE = 8192 samples warms up over the DC_WARM = 2048 samples before it (x_prev exact) and is checked at
      its start against its predecessor's end state (dc_chainup_kernel).

The rule of agreement is iir_states_agree: bit equality, or both below 2^-100 where the channel's gain allows it (WBFM: K >= 1,
DC removal: |gain| <= 1e6).  Everything here is numpy binary32, one rounding per operation, denormals kept; the exact states
come from the oracle's stage getters (wbfm_stages / dc_stages), i.e. from the serial recurrence over the whole stream.

A hand-off is `bad` when the warmed-up state differs from the EXACT state: each of them costs the device at least one re-run,
so a call's `state_repairs` rises by at least their number (tile kernel: by exactly their number; streamed launches re-run
the segment behind a re-run one as well).  What the device's first look FLAGS is a little different - it compares with the
predecessor's own record, which for an interior predecessor is itself the end of a zero-state run - and that is what
`state_checks` counts: hand-offs minus flagged ones.  Both are computed."""
import ctypes as C

import numpy as np

f32 = np.float32
TINY = 2.0 ** -100


def agree(a, b, tiny_ok=True):
    """iir_states_agree (iqd_wbfm.h) on scalars"""
    a, b = f32(a), f32(b)
    return a.tobytes() == b.tobytes() or (bool(tiny_ok) and abs(float(a)) < TINY and abs(float(b)) < TINY)


def agree_v(a, b, tiny_ok):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    same = a.view(np.uint32) == b.view(np.uint32)
    if not tiny_ok:
        return same
    return same | ((np.abs(a.astype(np.float64)) < TINY) & (np.abs(b.astype(np.float64)) < TINY))


def iir_run(u, a1, y, up, g0, n):
    """n steps of IQD_IIR_STEP over u from global sample g0 (u = 0 before the stream's start), one state"""
    a1 = f32(a1)
    for g in range(g0, g0 + n):
        x = u[g] if g >= 0 else f32(0)
        tn = f32(x + up)
        r = f32(a1 * y)
        y = f32(tn - r)
        up = x
    return y, up


def _take(x, idx):
    """x[idx] with zeros before the stream's start"""
    idx = np.asarray(idx, np.int64)
    return np.where(idx >= 0, x[np.clip(idx, 0, len(x) - 1)], f32(0)).astype(f32)


def iir_cold(u, a1, starts, steps):
    """The de-emphasis from the ZERO state at each of `starts`, `steps[i]` steps each -> the states y after them (all
    trajectories advance together; a finished one holds)."""
    starts = np.asarray(starts, np.int64)
    steps = np.broadcast_to(np.asarray(steps, np.int64), starts.shape)
    y, up = np.zeros(len(starts), f32), np.zeros(len(starts), f32)
    a1 = f32(a1)
    with np.errstate(under="ignore"):
        for j in range(int(steps.max()) if len(starts) else 0):
            x = _take(u, starts + j)
            yn = ((x + up).astype(f32) - (a1 * y).astype(f32)).astype(f32)
            live = j < steps
            y = np.where(live, yn, y)
            up = np.where(live, x, up)
    return y


def dc_cold(x, a1, starts, steps):
    """The DC-removal recurrence from y = 0 with the exact x_prev at each of `starts` (all >= 1)"""
    starts = np.asarray(starts, np.int64)
    steps = np.broadcast_to(np.asarray(steps, np.int64), starts.shape)
    y, xp = np.zeros(len(starts), f32), x[starts - 1].astype(f32)
    a1 = f32(a1)
    with np.errstate(under="ignore"):
        for j in range(int(steps.max()) if len(starts) else 0):
            xv = x[np.minimum(starts + j, len(x) - 1)].astype(f32)
            yn = ((xv - xp).astype(f32) - (a1 * y).astype(f32)).astype(f32)
            live = j < steps
            y = np.where(live, yn, y)
            xp = np.where(live, xv, xp)
    return y


def dc_serial(x, a1):
    """the plain recurrence over a whole stream from the zero state (what pins the oracle's detector-stream getter)"""
    y, xp, a1 = f32(0), f32(0), f32(a1)
    out = np.zeros(len(x), f32)
    with np.errstate(under="ignore"):
        for i, xv in enumerate(x.astype(f32)):
            y = f32(f32(xv - xp) - f32(a1 * y))
            xp = xv
            out[i] = y
    return out


_CONSTS = {}


def consts(L):
    """the kernels' own constants through the emulation library"""
    if not _CONSTS:
        L.emu_plan_const.restype = C.c_uint32
        L.emu_dc_a1.restype = C.c_float
        L.emu_restart_consts.restype = None
        L.emu_restart_consts.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
        c6, ab, k = np.zeros(6, np.uint32), np.zeros(2, f32), C.c_float(0)
        L.emu_restart_consts(c6.ctypes.data, ab.ctypes.data, 1.0, C.byref(k))
        _CONSTS.update(ST_HALO=int(L.emu_plan_const(2)), DC_TILE=int(L.emu_plan_const(3)), COLD_HALO=int(L.emu_plan_const(4)),
                       DC_WARM=int(L.emu_plan_const(5)), FORCED_BACK=int(L.emu_plan_const(6)), dc_a1=f32(L.emu_dc_a1()),
                       a1=f32(ab[0]), b0=f32(ab[1]))
    return _CONSTS


def wbfm_k(L, gain):
    """the K the engine derives from a WBFM demodulator gain"""
    L.emu_restart_consts.restype = None
    L.emu_restart_consts.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]   # (every CDLL object has its own prototypes)
    c6, ab, k = np.zeros(6, np.uint32), np.zeros(2, f32), C.c_float(0)
    L.emu_restart_consts(c6.ctypes.data, ab.ctypes.data, float(f32(gain)), C.byref(k))
    return f32(k.value)


DEFAULT_WBFM_GAIN = f32(256000 / (2 * np.pi))


def rotated(oracle, u8, rotation):
    s8 = (np.ascontiguousarray(u8, np.uint8) ^ 0x80).view(np.int8)
    return np.concatenate([oracle.rotate(s8[o:o + 32768], rotation) for o in range(0, len(s8), 32768)])


class Deemph:
    """One WBFM channel's whole stream (the samples its demodulator sees: closed blocks already taken out)."""

    def __init__(self, L, oracle, u8, rotation=1, gain=None):
        self.c = consts(L)
        self.gain = DEFAULT_WBFM_GAIN if gain is None else f32(gain)
        self.k = wbfm_k(L, self.gain)
        self.a1, self.b0 = self.c["a1"], self.c["b0"]
        st = oracle.wbfm_stages(rotated(oracle, u8, rotation), float(self.gain))
        self.u = (self.b0 * (self.k * st["dtheta"].astype(f32)).astype(f32)).astype(f32)   # b0 * (K * d), each product rounded
        self.y = st["deemph"].astype(f32)                                                  # exact state after sample n
        self.tiny_ok = bool(self.k >= f32(1.0))

    def exact(self, P):
        P = np.asarray(P, np.int64)
        return _take(self.y, P - 1)

    def where(self, form):
        """(zero-state steps before the comparison, how far before the boundary it is made)"""
        if form == "stream":
            return self.c["ST_HALO"], 0
        return self.c["COLD_HALO"] - self.c["FORCED_BACK"], self.c["FORCED_BACK"]

    def bad(self, bounds, form):
        """the boundaries (global samples) whose zero-state warm-up does not land on the exact state"""
        bounds = np.asarray(bounds, np.int64)
        lead, off = self.where(form)
        got = iir_cold(self.u, self.a1, bounds - off - lead, lead)
        return [int(b) for b, ok in zip(bounds, agree_v(got, self.exact(bounds - off), self.tiny_ok)) if not ok]

    def bad_by_the_plain_rule(self, bounds, lead):
        """`lead` zero-state steps ending AT the boundary against the exact state entering it"""
        bounds = np.asarray(bounds, np.int64)
        got = iir_cold(self.u, self.a1, bounds - lead, lead)
        return [int(b) for b, ok in zip(bounds, agree_v(got, self.exact(bounds), self.tiny_ok)) if not ok]

    def flagged(self, start, bounds, form):
        """what the device's first look flags in a call that starts at global sample `start` with the boundaries `bounds`: a
        segment's warmed-up state against its predecessor's own record (exact only for the call's first segment)"""
        bounds = np.asarray(bounds, np.int64)
        if not len(bounds):
            return []
        lead, off = self.where(form)
        got = iir_cold(self.u, self.a1, bounds - off - lead, lead)
        full = lead + off                                        # the predecessor's own zero-state run began `full` before ITS start
        prev_start = np.concatenate([[start], bounds[:-1]])
        want = iir_cold(self.u, self.a1, prev_start - full, bounds - off - (prev_start - full))
        want[0] = self.exact(bounds[:1] - off)[0]                # the call's first segment ran from the carried exact state
        return [int(b) for b, ok in zip(bounds, agree_v(got, want, self.tiny_ok)) if not ok]


class DcRemoval:
    """One AM / SSB channel's whole stream at 8 kS/s."""

    def __init__(self, L, oracle, u8, mode, rotation=1, gain=300.0):
        self.c = consts(L)
        st = oracle.dc_stages(rotated(oracle, u8, rotation), mode)
        self.x, self.y = st["det"], st["dc"]
        self.gain = f32(gain)
        self.tiny_ok = bool(abs(self.gain) <= f32(1e6))
        self.a1 = self.c["dc_a1"]

    def bounds(self, start, n):
        """tile boundaries (global 8 kS/s samples) of a call of n PCM samples that starts at `start`; none for a one-tile row"""
        return [start + b for b in range(self.c["DC_TILE"], n, self.c["DC_TILE"])]

    def bad(self, bounds):
        bounds = np.asarray(bounds, np.int64)
        if not len(bounds):
            return []
        got = dc_cold(self.x, self.a1, bounds - self.c["DC_WARM"], self.c["DC_WARM"])
        return [int(b) for b, ok in zip(bounds, agree_v(got, self.y[bounds - 1], self.tiny_ok)) if not ok]

    def flagged(self, start, bounds):
        bounds = np.asarray(bounds, np.int64)
        if not len(bounds):
            return []
        W = self.c["DC_WARM"]
        got = dc_cold(self.x, self.a1, bounds - W, W)
        prev_start = np.concatenate([[start], bounds[:-1]])
        want = self.y[bounds - 1].copy()
        if len(bounds) > 1:
            want[1:] = dc_cold(self.x, self.a1, prev_start[1:] - W, bounds[1:] - (prev_start[1:] - W))
        return [int(b) for b, ok in zip(bounds, agree_v(got, want, self.tiny_ok)) if not ok]


def squelch_chain(oracle, threshold, rotation=1):
    """an oracle chain that only runs the squelch (no demodulator): one per channel, kept over the channel's calls - the squelch
    remembers the block before"""
    o = oracle.chain()
    o.set_mode("none")
    o.set_rotation(rotation)
    o.set_squelch(threshold)
    return o


def open_samples(chain, u8, block_bytes):
    """What a squelch-gated channel's demodulator sees of a row: (the bytes of its open blocks, the `allowed` flags)."""
    _, _, allowed = chain.accept_stream(u8, block_bytes)
    blocks = np.ascontiguousarray(u8, np.uint8).reshape(-1, block_bytes)
    return blocks[allowed.astype(bool)].reshape(-1), allowed
