"""CPU tier: a step model of the WBFM streaming kernel's y2 ring - the LDS ring through which an IIR wave hands each piece's
pair of stage-2 outputs to the audio wave (iqd_stream.hip: st_iir_piece, st_audio_piece).

What runs REAL code: where a piece lives and who may touch it when - `st_y2_piece` of iqd_stream.h, the one function both
waves call, compiled for the host (tests/emu/emu_y2_ring.cpp).  What is MODELLED: the two waves as single-threaded programs of
three steps per piece, each step atomic, as on the device (a wave's LDS operations reach the LDS in program order, and each
side fences between its data access and its counter update):

    IIR wave   (1) wait until `consumed` has reached need_consumed   (2) write the slot   (3) add add_full to `full`
    audio wave (1) wait until `full` has reached need_full           (2) read the slot    (3) add 1 to `consumed`

with the piece counters running on through the rounds, as the waves' do.  EVERY interleaving of the two programs is walked
(the state is the pair of program counters; a waiting step that may not pass does not move).  Three assertions: no slot is
written before its previous content was read, none is read before the piece it is read for was written, and from every
reachable state somebody can move until both are done - a wrong wait condition would be a hang on the device.

The test has teeth: each of the three assertions is shown to fire on a wait condition that is off by one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("y2ring") / "libiqd_y2_ring.so")
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-Wall",
                    "-I" + os.path.join(ROOT, "rtlsdrdiags_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(HERE, "emu", "emu_y2_ring.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.emu_st_y2_piece.restype = None
    L.emu_st_y2_piece.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.emu_st_y2_ring_ok.restype = C.c_int
    L.emu_st_y2_ring_ok.argtypes = [C.c_uint32, C.c_uint32]
    L.emu_st_y2_consts.restype = None
    L.emu_st_y2_consts.argtypes = [C.c_void_p]
    return L


def real_piece(L):
    def piece(k, depth, every):
        out = np.zeros(4, np.uint32)
        L.emu_st_y2_piece(k & 0xffffffff, depth, every, out.ctypes.data)
        return tuple(int(v) for v in out)       # slot, need_consumed, need_full, add_full
    return piece


def reached(counter, need):
    """(int32_t)(counter - need) >= 0, as the kernel compares"""
    return ((counter - need) & 0xffffffff) < 0x80000000


class Hang(AssertionError):
    pass


def walk(piece, depth, every, rounds, first_piece=0):
    """Every interleaving of the two programs over sum(rounds) pieces.  Returns the number of states visited."""
    n = sum(rounds)
    plan = [piece((first_piece + k) & 0xffffffff, depth, every) for k in range(n)]
    for slot, _, _, _ in plan:
        assert 0 <= slot < depth

    def state_of(pp, cp):
        """The ring and its counters when the IIR wave has done pp steps and the audio wave cp (counters start at first_piece,
        as if that many pieces had gone through before)."""
        full = first_piece + sum(plan[k][3] for k in range(pp // 3))
        consumed = first_piece + cp // 3
        return full & 0xffffffff, consumed & 0xffffffff

    seen, stack = set(), [(0, 0)]
    while stack:
        pp, cp = stack.pop()
        if (pp, cp) in seen:
            continue
        seen.add((pp, cp))
        full, consumed = state_of(pp, cp)
        moves = []
        if pp < 3 * n:
            k, step = divmod(pp, 3)
            slot, need_consumed, _, _ = plan[k]
            if step == 0:
                if reached(consumed, need_consumed):
                    moves.append((pp + 1, cp))
            elif step == 1:
                # the slot's previous content: the latest earlier piece of the same slot - its read must be over
                older = [j for j in range(k) if plan[j][0] == slot]
                if older:
                    assert cp >= 3 * older[-1] + 2, "piece %d overwrites piece %d in slot %d before it was read (D=%d, every=%d, rounds=%r)" % (
                        k, older[-1], slot, depth, every, rounds)
                moves.append((pp + 1, cp))
            else:
                moves.append((pp + 1, cp))
        if cp < 3 * n:
            j, step = divmod(cp, 3)
            slot, _, need_full, _ = plan[j]
            if step == 0:
                if reached(full, need_full):
                    moves.append((pp, cp + 1))
            elif step == 1:
                assert pp >= 3 * j + 2, "piece %d is read before it was written (D=%d, every=%d, rounds=%r)" % (j, depth, every, rounds)
                # ... and nothing later has been written over it
                later = [k for k in range(j + 1, n) if plan[k][0] == slot]
                assert not later or pp < 3 * later[0] + 2, "piece %d was overwritten by piece %d before it was read" % (j, later[0])
                moves.append((pp, cp + 1))
            else:
                moves.append((pp, cp + 1))
        if not moves and (pp < 3 * n or cp < 3 * n):
            raise Hang("both waves wait for ever at IIR step %d, audio step %d (full %d, consumed %d; D=%d, every=%d, rounds=%r)" % (
                pp, cp, full, consumed, depth, every, rounds))
        stack.extend(moves)
    assert (3 * n, 3 * n) in seen
    return len(seen)


DEPTHS = [1, 2, 4, 8]


def rounds_for(depth, every):
    """Two rounds each; piece counts that are and are not multiples of the depth.  A ring hands over whole groups of `every`
    pieces per round (the kernel: multiples of four), so with every = 4 the counts are multiples of four."""
    if every == 1:
        counts = [depth, 2 * depth, 3 * depth, 1, 3, 5, 7, 4 * depth + 1, 4 * depth + 3]
    else:
        counts = [4, 8, 12, 16, 20, 24]
    return [(a, b) for a in counts for b in counts]


@pytest.mark.parametrize("every", [1, 4])
@pytest.mark.parametrize("depth", DEPTHS)
def test_every_interleaving_of_the_hand_over(lib, depth, every):
    piece = real_piece(lib)
    if not lib.emu_st_y2_ring_ok(depth, every):
        # a ring that cannot hold a group of pieces: the header refuses to build it (static_assert on st_y2_ring_ok) - and
        # rightly: the IIR wave would wait for room before it has signalled anything
        assert depth < every
        with pytest.raises(Hang):
            walk(piece, depth, every, (8, 8))
        return
    n_states = 0
    some_multiple = some_other = False
    for rounds in rounds_for(depth, every):
        n_states += walk(piece, depth, every, rounds)
        some_multiple |= rounds[0] % depth == 0
        some_other |= rounds[0] % depth != 0
    assert some_multiple
    if depth > 1 and (every == 1 or depth > every):
        assert some_other
    assert n_states > 1000


@pytest.mark.parametrize("every", [1, 4])
def test_the_counters_wrap(lib, every):
    """The piece counters are 32-bit and compared as signed differences: a ring that has seen nearly 2^32 pieces goes on."""
    piece = real_piece(lib)
    for depth in (4, 8):
        walk(piece, depth, every, (12, 8), first_piece=(1 << 32) - 8)


def test_a_group_may_straddle_two_rounds(lib):
    """every = 4 with rounds of 6 + 6 pieces: the counters run on through the rounds, the third signal comes in the second."""
    piece = real_piece(lib)
    walk(piece, 4, 4, (6, 6))
    walk(piece, 8, 4, (6, 10))
    with pytest.raises(Hang):                      # ... but pieces that never complete a group are never seen
        walk(piece, 4, 4, (6, 4))


def test_the_shipped_ring(lib):
    c = np.zeros(8, np.uint32)
    lib.emu_st_y2_consts(c.ctypes.data)
    depth, every, ring_bytes, y2_off, sync_off, lds_bytes, w_full, w_consumed = (int(v) for v in c)
    assert lib.emu_st_y2_ring_ok(depth, every)
    assert ring_bytes == depth * 64 * 4
    assert sync_off == y2_off + 3 * ring_bytes and lds_bytes == sync_off + 24 * 4 and lds_bytes <= 160 * 1024
    assert {w_full, w_consumed} <= {5, 6, 7} and w_full != w_consumed      # the spare words of a ring's eight
    piece = real_piece(lib)
    for rounds in ((172, 196), (196, 196), (4, 196)):    # (a fast ring of the bench's segments hands over 172 pieces a round)
        walk(piece, depth, every, rounds)


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_the_model_catches_wait_conditions_that_are_off_by_one(lib, depth):
    piece = real_piece(lib)

    def early_write(k, d, e):
        slot, need_consumed, need_full, add_full = piece(k, d, e)
        return slot, (need_consumed - 1) & 0xffffffff, need_full, add_full

    def early_read(k, d, e):
        slot, need_consumed, need_full, add_full = piece(k, d, e)
        return slot, need_consumed, (need_full - 1) & 0xffffffff, add_full

    def late_write(k, d, e):
        slot, need_consumed, need_full, add_full = piece(k, d, e)
        return slot, (need_consumed + 1) & 0xffffffff, need_full, add_full

    with pytest.raises(AssertionError, match="overwrites"):
        walk(early_write, depth, 1, (9, 5))
    with pytest.raises(AssertionError, match="read before it was written"):
        walk(early_read, depth, 1, (9, 5))
    if depth == 1:
        with pytest.raises(Hang):
            walk(late_write, depth, 1, (9, 5))
    else:
        walk(late_write, depth, 1, (9, 5))             # (a deeper ring only loses a slot)
