/* Prints the layout of every public struct of include/iqdemod.h as the C compiler sees it: one line "struct <name> <sizeof>",
 * then one line "<name>.<field> <offsetof> <size>" per field, in the header's order.  tests/test_abi_layout.py holds the
 * lines against the header's own field lists and against the Python binding's mirrors.  Plain C99, no library. */
#include <stddef.h>
#include <stdio.h>

#include "iqdemod.h"

#define S(T) printf("struct %s %zu\n", #T, sizeof(T))
#define F(T, f) printf("%s.%s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T *)0)->f))

int main(void)
{
    S(iqd_config);
    F(iqd_config, abi_version); F(iqd_config, n_channels); F(iqd_config, block_bytes); F(iqd_config, device);
    F(iqd_config, flags); F(iqd_config, reserved);

    S(iqd_agc_state);
    F(iqd_agc_state, enabled); F(iqd_agc_state, type); F(iqd_agc_state, operating_point_dbfs); F(iqd_agc_state, deadband_db);
    F(iqd_agc_state, blanking_limit); F(iqd_agc_state, alpha); F(iqd_agc_state, rx_gain_db); F(iqd_agc_state, if_gain_db);
    F(iqd_agc_state, filtered_if_gain_db); F(iqd_agc_state, blanking_counter); F(iqd_agc_state, gain_was_adjusted);
    F(iqd_agc_state, normalized_level_dbfs); F(iqd_agc_state, signal_magnitude);

    S(iqd_stats);
    F(iqd_stats, accepts); F(iqd_stats, samples); F(iqd_stats, kernel_launches); F(iqd_stats, state_checks);
    F(iqd_stats, state_repairs); F(iqd_stats, chain_kernel_ms); F(iqd_stats, chain_kernel_count); F(iqd_stats, segment_repairs);
    F(iqd_stats, stream_launches); F(iqd_stats, device_launches); F(iqd_stats, device_copies); F(iqd_stats, mixed_launches);

    S(iqd_channelizer_config);
    F(iqd_channelizer_config, n_sources); F(iqd_channelizer_config, n_channels); F(iqd_channelizer_config, decimation);
    F(iqd_channelizer_config, n_taps); F(iqd_channelizer_config, taps); F(iqd_channelizer_config, decimation_den);
    F(iqd_channelizer_config, sample_format); F(iqd_channelizer_config, reserved);

    S(iqd_spectrum_config);
    F(iqd_spectrum_config, n_sources); F(iqd_spectrum_config, n_bins); F(iqd_spectrum_config, window);
    F(iqd_spectrum_config, sample_format); F(iqd_spectrum_config, reserved);

    S(iqd_detect_config);
    F(iqd_detect_config, n_bins); F(iqd_detect_config, floor_rank); F(iqd_detect_config, ratio_q8); F(iqd_detect_config, dc_guard);
    F(iqd_detect_config, bridge); F(iqd_detect_config, min_width); F(iqd_detect_config, max_detections);
    F(iqd_detect_config, reserved);

    S(iqd_detect_row);
    F(iqd_detect_row, floor); F(iqd_detect_row, threshold); F(iqd_detect_row, n_found); F(iqd_detect_row, n_hot_bins);

    S(iqd_detection);
    F(iqd_detection, first_bin); F(iqd_detection, last_bin); F(iqd_detection, peak_bin); F(iqd_detection, peak_power);
    F(iqd_detection, sum_power); F(iqd_detection, centroid_q8); F(iqd_detection, n_hot);

    S(iqd_track_config);
    F(iqd_track_config, n_sources); F(iqd_track_config, n_bins); F(iqd_track_config, max_detections); F(iqd_track_config, n_slots);
    F(iqd_track_config, gate_q8); F(iqd_track_config, open_hits); F(iqd_track_config, hold_blocks); F(iqd_track_config, alpha_q8);
    F(iqd_track_config, inc_bias); F(iqd_track_config, class_edge); F(iqd_track_config, reserved);

    S(iqd_track_slot);
    F(iqd_track_slot, track_id); F(iqd_track_slot, state); F(iqd_track_slot, flags); F(iqd_track_slot, hits);
    F(iqd_track_slot, width_class); F(iqd_track_slot, misses); F(iqd_track_slot, max_width); F(iqd_track_slot, centre_q8);
    F(iqd_track_slot, phase_inc); F(iqd_track_slot, first_bin); F(iqd_track_slot, last_bin); F(iqd_track_slot, peak_power);
    F(iqd_track_slot, age_blocks);

    S(iqd_track_block);
    F(iqd_track_block, n_active); F(iqd_track_block, n_tentative); F(iqd_track_block, n_opened_closed); F(iqd_track_block, n_unplaced);

    S(iqd_track_follow);
    F(iqd_track_follow, slots_dev); F(iqd_track_follow, n_slots); F(iqd_track_follow, n_blocks); F(iqd_track_follow, block_bytes);
    F(iqd_track_follow, lag); F(iqd_track_follow, min_state); F(iqd_track_follow, reserved);

    S(iqd_measure_config);
    F(iqd_measure_config, n_sources); F(iqd_measure_config, n_bins); F(iqd_measure_config, n_slots); F(iqd_measure_config, dc_guard);
    F(iqd_measure_config, margin); F(iqd_measure_config, obw_tail_q16); F(iqd_measure_config, carrier_half);
    F(iqd_measure_config, min_sum); F(iqd_measure_config, carrier_min_q8); F(iqd_measure_config, wide_bins);
    F(iqd_measure_config, reserved);

    S(iqd_track_measure);
    F(iqd_track_measure, track_id); F(iqd_track_measure, obw_lo); F(iqd_track_measure, obw_hi); F(iqd_track_measure, peak_bin);
    F(iqd_track_measure, flags); F(iqd_track_measure, hint); F(iqd_track_measure, peak_excess); F(iqd_track_measure, centroid_q8);
    F(iqd_track_measure, carrier_q8); F(iqd_track_measure, n_over); F(iqd_track_measure, sum_excess);

    S(iqd_tracklog_config);
    F(iqd_tracklog_config, n_sources); F(iqd_tracklog_config, n_slots); F(iqd_tracklog_config, max_events);
    F(iqd_tracklog_config, min_active); F(iqd_tracklog_config, vote_min); F(iqd_tracklog_config, reserved);

    S(iqd_track_summary);
    F(iqd_track_summary, track_id); F(iqd_track_summary, state); F(iqd_track_summary, flags); F(iqd_track_summary, mode_hint);
    F(iqd_track_summary, width_class); F(iqd_track_summary, first_block); F(iqd_track_summary, n_blocks); F(iqd_track_summary, n_active);
    F(iqd_track_summary, n_measured); F(iqd_track_summary, votes); F(iqd_track_summary, sum_centre_q8); F(iqd_track_summary, sum_excess);
    F(iqd_track_summary, peak_excess); F(iqd_track_summary, obw_lo_min); F(iqd_track_summary, obw_hi_max);

    S(iqd_tracklog_counts);
    F(iqd_tracklog_counts, n_events); F(iqd_tracklog_counts, n_stored); F(iqd_tracklog_counts, n_short); F(iqd_tracklog_counts, n_lost);
    return 0;
}
