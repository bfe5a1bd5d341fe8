// tests/emu - TEST INFRASTRUCTURE ONLY: the y2 ring's slot / counter arithmetic (iqd_stream.h: st_y2_piece, the one function both
// sides of the WBFM streaming kernel's IIR-wave -> audio-wave hand-over use) compiled for the host, for
// tests/test_emu_y2_ring_model.py.  A library of its own: it needs nothing but the header.
#include <stdint.h>

#include "iqd_stream.h"

using namespace iqd;

extern "C" {

// out4 = slot, need_consumed, need_full, add_full
void emu_st_y2_piece(uint32_t piece, uint32_t depth, uint32_t every, uint32_t *out4)
{
    const StY2Piece p = st_y2_piece(piece, depth, every);
    out4[0] = p.slot;
    out4[1] = p.need_consumed;
    out4[2] = p.need_full;
    out4[3] = p.add_full;
}

int emu_st_y2_ring_ok(uint32_t depth, uint32_t every) { return st_y2_ring_ok(depth, every) ? 1 : 0; }

// out8 = the shipped depth and signal period, bytes of one ring, offset of the rings, offset of the counters, LDS bytes of the
// kernel, the two counters' words within a ring's eight
void emu_st_y2_consts(uint32_t *out8)
{
    out8[0] = ST_Y2_DEPTH;
    out8[1] = ST_Y2_EVERY;
    out8[2] = ST_Y2_RING_BYTES;
    out8[3] = ST_Y2_OFF;
    out8[4] = ST_SYNC_OFF;
    out8[5] = ST_LDS_BYTES;
    out8[6] = ST_SYNC_Y2_FULL;
    out8[7] = ST_SYNC_Y2_CONSUMED;
}

}
