// The band spectrum (include/iqdemod.h: "Band spectrum"): what iqd_spectrum.cpp and iqd_spectrum.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace iqd {

// A workgroup is SPC_WAVES waves on the same frames, one tile of SPC_TILE_BINS bins each; a wave takes its block's frames
// SPC_CHUNK at a time (SPC_CHUNK / 16 MFMA tiles of 16 frames).
constexpr uint32_t SPC_WAVES = 4, SPC_TILE_BINS = 16, SPC_WG_BINS = SPC_WAVES * SPC_TILE_BINS;
constexpr uint32_t SPC_FRAME_TILES = 4, SPC_CHUNK = 16 * SPC_FRAME_TILES;
constexpr uint32_t SPC_MIN_BINS = 64, SPC_MAX_BINS = 2048, SPC_MAX_FRAMES = 1u << 24;
// A operand planes of a bin tile, in this order: rail r (c, s, ...) low and high byte plane, rail i (-s, c, ...) likewise
constexpr uint32_t SPC_PLANES = 4;

// amat: [N / 16 bin tiles][N / 32 K steps][SPC_PLANES][64 lanes] 16-byte operands, 8 N^2 bytes: lane rho + 16 g holds bytes
// kappa = 64 step + 16 g + j, j < 16, of row rho of the tile, kappa = 2 n + (0: the I rail, 1: the Q rail).
inline size_t spc_amat_bytes(uint32_t n) { return (size_t)8 * n * n; }
void spc_pack(const int16_t *window, const int16_t *phasor /* [8192] */, uint32_t n, uint8_t *amat);

struct SpcLaunch {
    const uint8_t *wide;   // [n_sources][bytes_per_source]
    uint32_t *power;       // [n_sources][n_blocks][n]
    const uint4 *amat;
    size_t bytes_per_source;
    uint32_t n, n_sources, n_blocks, frames;   // frames: F
    uint32_t flip;         // offset binary: every byte ^ 0x80
};
hipError_t launch_spectrum(const SpcLaunch &a, hipStream_t s);

}  // namespace iqd
