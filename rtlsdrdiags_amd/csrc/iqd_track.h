// The band activity tracker (include/iqdemod.h: "Band tracks"): what iqd_track.cpp and iqd_track.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace iqd {

// A wave owns a source and is a workgroup by itself; lane s is slot s.  Nothing crosses from wave to wave.
constexpr uint32_t TRK_MAX_SLOTS = 64;
constexpr uint32_t TRK_MIN_BINS = 64, TRK_MAX_BINS = 2048;
constexpr uint32_t TRK_MAX_OPEN = 255, TRK_MAX_HOLD = 65535, TRK_MAX_ALPHA = 256;
constexpr size_t TRK_MAX_ROWS = 0x7fffffffull;            // n_sources x n_blocks of one call
constexpr uint32_t TRK_SLOT_BYTES = 32, TRK_BLOCK_BYTES = 16;

struct TrkLaunch {
    const uint4 *rows;       // [n_sources][n_blocks] iqd_detect_row
    const uint4 *det;        // [n_sources][n_blocks][max_det] iqd_detection, two 16-byte halves each
    uint4 *slots;            // [n_sources][n_blocks][n_slots] iqd_track_slot, two 16-byte halves each
    uint4 *blocks;           // [n_sources][n_blocks] iqd_track_block
    uint4 *state;            // [n_sources][n_slots] iqd_track_slot: read at the call's start, written at its end
    uint32_t *next_id;       // [n_sources]
    size_t n_blocks;
    uint32_t n_sources, n, max_det, n_slots, gate, open_hits, hold, alpha, inc_bias, edge0, edge1, edge2;
};
hipError_t launch_track(const TrkLaunch &a, hipStream_t s);

}  // namespace iqd
