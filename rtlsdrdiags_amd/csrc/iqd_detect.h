// The band activity detector (include/iqdemod.h: "Band activity"): what iqd_detect.cpp and iqd_detect.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace iqd {

// A wave owns a row; a workgroup is DET_WAVES waves on DET_WAVES consecutive rows, each with its own slice of LDS (the
// row and the radix select's 256 counters).  Nothing crosses from wave to wave.
constexpr uint32_t DET_WAVES = 4;
constexpr uint32_t DET_MIN_BINS = 64, DET_MAX_BINS = 2048, DET_MAX_BRIDGE = 64;
constexpr uint32_t DET_MIN_RATIO = 256, DET_MAX_RATIO = 1u << 24;
constexpr size_t DET_MAX_ROWS = 0x7fffffffull;            // of one launch
constexpr uint32_t DET_ROW_BYTES = 16, DET_RECORD_BYTES = 32;

struct DetLaunch {
    const uint32_t *power;   // [n_rows][n]
    uint4 *rows;             // [n_rows] iqd_detect_row
    uint4 *det;              // [n_rows][max_det] iqd_detection, two 16-byte halves each
    size_t n_rows;
    uint32_t n, rank, ratio_q8, dc_guard, bridge, min_width, max_det;
};
hipError_t launch_detect(const DetLaunch &a, hipStream_t s);

}  // namespace iqd
