// Wideband channelizer (include/iqdemod.h: iqd_channelizer_*): launch descriptor of the gfx950 kernel and the host-only
// pieces of its integer spec, shared by iqd_chan.hip (device) and iqd_chan.cpp (host orchestration).
//
// Per source the filter is a GEMM on v_mfma_i32_16x16x64_i8: A = (8 channels x {Ar, Ai}) x (2 Kp bytes of window),
// B = (2 Kp bytes) x (16 outputs), the sliding window over the source's interleaved signed bytes.  Kp = K rounded up to
// 32 samples (the taps of k >= K are 0), so that a window is a whole number of 64-byte K-chunks.  K-index kappa of a
// window (0 = oldest byte) is sample k = Kp - 1 - kappa / 2, rail kappa & 1 (I, Q).  Row 2 l + 0 of a tile (channel l)
// holds gr[k] on I and -gi[k] on Q, row 2 l + 1 gi[k] on I and gr[k] on Q; every int16 tap t = 256 hi + lo is split
// into two signed-byte planes, each plane one MFMA, combined exactly in the epilogue.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "iqdemod.h"

namespace iqd {

constexpr uint32_t CHZ_TILE_CH = 8;          // channels per 16-row MFMA tile (one wave)
constexpr uint32_t CHZ_WAVES = 8;            // tiles (waves) per workgroup, all of one source
constexpr uint32_t CHZ_GROUP = 64;           // outputs per store group: 8 channels x 128 bytes = one 16-byte store per lane
constexpr uint32_t CHZ_PHASOR = 4096;
constexpr uint32_t CHZ_WIN_MAX = 32768;      // LDS bytes of a workgroup's window
constexpr uint32_t CHZ_LDS_FIXED = CHZ_PHASOR * 4 + CHZ_WAVES * CHZ_TILE_CH * 2 * CHZ_GROUP;   // phasor + output staging
constexpr uint32_t CHZ_NQ_REG = 8;           // up to this many K-chunks the A operands stay in registers
constexpr uint32_t CHZ_NONE = 0xffffffffu;   // a padding slot of a tile

struct ChzTile {
    uint32_t ch[CHZ_TILE_CH];       // output row per slot, CHZ_NONE = padding (its taps are 0, nothing is stored)
    uint32_t inc[CHZ_TILE_CH];      // phase increment d_c
    uint32_t shift[CHZ_TILE_CH];    // gain shift L_c
};

struct ChzWg {                       // one workgroup row of the grid: up to CHZ_WAVES tiles of one source
    uint32_t source, first_tile, n_tiles, pad;
};

struct ChzLaunch {
    const uint8_t *wide;             // [n_sources][bytes_per_source] offset-binary I/Q, 16-byte aligned
    const uint8_t *hist;             // [n_sources][2 kp] raw bytes of samples [-kp, 0) of this call
    uint8_t *hist_next;              // the same after this call
    const uint32_t *phasor;          // [4096]: (uint16)c | s << 16
    const uint4 *amat;               // [n_tiles][nq][2 planes][64 lanes] A operands
    const ChzTile *tiles;
    const ChzWg *wgs;
    uint8_t *out;                    // [n_ch][out_row]
    size_t bytes_per_source;
    uint32_t n_sources, out_row, n_out, m, kp, nq, t_blk;
    uint32_t nbase;                  // (outputs before this call * M) mod 2^32
};

hipError_t launch_channelizer(const ChzLaunch &a, uint32_t n_wgs, hipStream_t s);

// host-only spec pieces (iqd_chan.cpp)
void chz_phasor_table(int16_t *out /* [8192] (c, s) pairs */);
// complex taps of one channel: gr, gi [K]
void chz_channel_taps(const int16_t *h, uint32_t k, uint32_t inc, const int16_t *phasor, int16_t *gr, int16_t *gi);

// the engine's side (iqd_engine.cpp)
int engine_fail(iqd_t *e, int code, const char *msg);
void engine_geometry(const iqd_t *e, uint32_t *n_ch, uint32_t *block_bytes, uint32_t *flags);

}  // namespace iqd
