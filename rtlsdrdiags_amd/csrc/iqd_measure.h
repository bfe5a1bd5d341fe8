// Band track measurements (include/iqdemod.h: "Band track measurements"): what iqd_measure.cpp and iqd_measure.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace iqd {

// A workgroup of MSR_WAVES waves owns one (source, block): its power row becomes two prefix arrays in LDS, then the row's S
// slots are spread over the waves.
constexpr uint32_t MSR_WAVES = 4;
constexpr uint32_t MSR_MAX_SLOTS = 64;
constexpr uint32_t MSR_MIN_BINS = 64, MSR_MAX_BINS = 2048;
constexpr uint32_t MSR_MAX_MARGIN = 64, MSR_MAX_BETA = 32767, MSR_MAX_CARRIER_HALF = 8, MSR_MAX_CARRIER_Q8 = 256;
constexpr size_t MSR_MAX_ROWS = 0x7fffffffull;            // n_sources x n_blocks of one call: one workgroup each
constexpr uint32_t MSR_RECORD_BYTES = 32;

struct MsrLaunch {
    const uint32_t *power;   // [n_sources][n_blocks][n]
    const uint4 *rows;       // [n_sources][n_blocks] iqd_detect_row
    const uint4 *slots;      // [n_sources][n_blocks][n_slots] iqd_track_slot, two 16-byte halves each
    uint4 *meas;             // [n_sources][n_blocks][n_slots] iqd_track_measure, two 16-byte halves each
    size_t n_rows;           // n_sources x n_blocks
    uint32_t n, n_slots, dc_guard, margin, beta, carrier_half, min_sum, carrier_min, wide_bins;
};
hipError_t launch_measure(const MsrLaunch &a, hipStream_t s);

}  // namespace iqd
