// PCM tone bank (include/iqdemod_tones.h): what iqd_tones.cpp and iqd_tones.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace iqd {

constexpr uint32_t TON_MIN_L = 32, TON_MAX_L = 8192, TON_MAX_T = 64;
constexpr uint32_t TON_TILE_CH = 16;       // channels of one workgroup: the MFMA tile's columns
constexpr uint32_t TON_TILE_ROWS = 16;     // rows of one MFMA tile: 8 tones x (c, s), row 2 t' = c, 2 t' + 1 = s
constexpr uint32_t TON_WAVES = 4;          // wave w of a workgroup runs row tiles w and w + 4
constexpr uint32_t TON_KC = 1024;          // samples of a frame staged in LDS at a time
constexpr uint32_t TON_RECORD_BYTES = 40, TON_STATE_BYTES = 32;
constexpr size_t TON_MAX_N = 0x7fffffffull;

// A frame's samples padded with zeros to a whole number of 64-sample K-chunks
constexpr uint32_t ton_padded(uint32_t L) { return (L + 63u) & ~63u; }
constexpr uint32_t ton_row_tiles(uint32_t T) { return (2 * T + TON_TILE_ROWS - 1) / TON_TILE_ROWS; }

// one channel's carried state (iqd_tones_state's bytes)
struct TonState {
    int32_t tone, cand;
    uint32_t run, miss, fill;
    uint32_t reserved[3];
};

struct TonLaunch {
    // the object's
    const uint4 *amat;       // A operands: [row tile][K-chunk][plane: 0 = hi, 1 = lo'][64 lanes] x 16 bytes (ton_pack, iqd_tones.cpp)
    const int32_t *gsum;     // [row tiles x 16]: a row's coefficient sum
    TonState *state;         // [n_channels]
    int16_t *open;           // [n_channels][L]: the open frame's samples
    uint32_t n_channels, L, T;
    uint64_t min_power;
    uint32_t ratio_q8, energy_q8, open_frames, hold;
    // the call's
    const int16_t *pcm;
    const uint32_t *count;   // or NULL
    size_t row_stride;
    uint32_t n, F;
    uint32_t *n_frames;
    uint64_t *frames;        // [n_channels][F] records of five uint64
    uint64_t *power;         // or NULL
};
hipError_t launch_tones_frames(const TonLaunch &a, hipStream_t s);   // every record up to the decision; F >= 1
hipError_t launch_tones_close(const TonLaunch &a, hipStream_t s);    // the decision, the counts, the carry
hipError_t launch_tones_reset(TonState *state, uint32_t n_channels, hipStream_t s);   // tone = cand = -1, the rest 0

}  // namespace iqd
