// The band track log (include/iqdemod.h: "Band track log"): what iqd_tracklog.cpp and iqd_tracklog.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace iqd {

// A wave owns a source and is a workgroup by itself; lane s is slot s.  Nothing crosses from wave to wave.
constexpr uint32_t TLG_MAX_SLOTS = 64;
constexpr uint32_t TLG_MAX_EVENTS = 65536, TLG_MAX_MIN_ACTIVE = 65535, TLG_MAX_VOTE_MIN = 65535;
constexpr size_t TLG_MAX_ROWS = 0x7fffffffull;            // n_sources x n_blocks of one call
constexpr uint32_t TLG_SUMMARY_BYTES = 64, TLG_COUNTS_BYTES = 16;

struct TlgLaunch {
    const uint4 *slots;      // [n_sources][n_blocks][n_slots] iqd_track_slot, two 16-byte halves each (the first is read)
    const uint4 *meas;       // [n_sources][n_blocks][n_slots] iqd_track_measure, two 16-byte halves each
    uint4 *summary;          // [n_sources][n_blocks][n_slots] iqd_track_summary, four 16-byte quarters each
    uint4 *events;           // [n_sources][max_events] iqd_track_summary
    uint4 *counts;           // [n_sources] iqd_tracklog_counts
    uint4 *state;            // [n_sources][n_slots] iqd_track_summary: read at the call's start, written at its end
    uint64_t *g;             // [n_sources] the source's absolute block index
    size_t n_blocks;
    uint32_t n_sources, n_slots, max_events, min_active, vote_min;
};
hipError_t launch_tracklog(const TlgLaunch &a, hipStream_t s);

}  // namespace iqd
