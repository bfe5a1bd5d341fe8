// The engine behind the C ABI (include/iqdemod.h), for the translation units that implement it: iqd_engine.cpp (lifecycle,
// setters, AGC, scanner, traces, stats), iqd_accept.cpp (the accept path), iqd_resampler.cpp and iqd_devmem.cpp.  Internal:
// the channelizer (iqd_chan.cpp, iqd_chan_survey.cpp) talks to the engine through the shims of iqd_chan.h and does not see this struct.
#pragma once
#include "iqdemod.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "iqd_hipres.h"
#include "iqd_host.h"
#include "iqd_plan.h"
#include "iqd_kernels.h"
#include "iqd_stream.h"
#include "iqd_stream_mixed.h"
#include "iqd_taps.h"
#include "iqd_wbfm.h"
#include "iqd_chains.h"

using namespace iqd;

// (the streaming thresholds STREAM_MIN_SEG_* and every tile / stream / one-launch decision: iqd_plan.h, iqd_plan.cpp)

struct iqd_engine {
    std::mutex mu;             // parameter mirror + dirty flags (setters vs. accept)
    int device = 0;
    Stream stream;
    uint32_t n_ch = 0, block_bytes = 0, block_samples = 0, flags = 0;
    Consts consts;

    std::vector<ChanParams> h_params;
    bool params_dirty = true;
    bool lists_dirty = true;
    uint32_t list_first = 0, list_n = 0;
    std::vector<uint32_t> h_lists[FAM_COUNT + 1];  // per family; [FAM_COUNT] = mode None
    uint32_t rot_count[FAM_COUNT][3] = {};         // channels of each family per rotation group (+Fs/4, none, -Fs/4)
    uint32_t n_cus = 256;
    // iqd_config::flags and the measurement knobs, read from the environment ONCE at creation (include/iqdemod.h): what
    // plan_call() decides from.  The plan of the last call is kept while the call's shape repeats (planning a
    // 2^28-sample FM + WBFM call cost more host time than its kernels run).
    PlanKnobs knobs;
    CallShape plan_shape;
    CallPlan plan;
    bool plan_valid = false;
    size_t dcr_layout[2][2] = {{~(size_t)0, 0}, {~(size_t)0, 0}};   // AM / SSB: where the DC redo flags sit in their buffer, and how many
    bool any_gated = false, any_agc = false;
    bool demod_bypass = false;             // inside iqd_demod_accept: the demodulator alone - no squelch, tracker, AGC, scanner, magnitudes
    std::vector<AgcConfig> h_agc;           // per channel; the one-shot fields are cleared once applied
    std::vector<uint8_t> agc_touched;       // the device may have moved this channel's IF gain
    bool agc_dirty = true;
    std::vector<ScanConfig> h_scan;         // per channel; one-shot fields cleared once applied
    std::vector<uint8_t> scan_new_cfg;      // FrequencyScanner::newConfigurationAvailable
    bool trace_on = false;
    uint32_t trace_first = 0, trace_n = 0, trace_blocks = 0;   // what gain_trace holds

    // persistent device state
    DevArray<ChanParams> d_params;
    DevArray<uint8_t> d_tails;
    DevArray<WbfmCarry> d_wcarry;
    DevArray<DcCarry> d_dc;
    DevArray<uint32_t> d_tracker;
    DevArray<AgcConfig> d_agc_cfg;
    DevArray<AgcState> d_agc;
    DevArray<GainEpoch> d_epochs;
    std::vector<float> k_applied;           // [n_ch][2]: the WBFM / FM K the device last ran with
    // [n_ch]: WBFM samples a channel still has to consume before its latest gain change is out of every lead-in's reach
    // (GainEpochList on the device; this mirror only decides which instantiation of the streaming kernel runs: the one
    // with the piecewise-gain lookup while any channel of the launch is non-zero here).  Never cleared early: it goes
    // down only by samples the channel's WBFM chain really consumed.
    std::vector<uint32_t> wbfm_epoch_left;
    // ... aged by arithmetic for ungated calls (every channel consumes the whole call); a squelch-gated call's consumption is
    // known to the device only, which then reports: its WBFM tail updates set word [0] of a page-locked pair if any
    // channel's newest change still lies inside its tail, a one-store kernel at the call's end writes the call's number to
    // word [1], and a later call that finds its number there and word [0] clear drops the mirror of that call's channels.
    std::vector<uint32_t> wbfm_epoch_seq;   // the first accept (accept_seq) whose chain ran with the channel's newest change
    uint32_t accept_seq = 0;
    PinnedArray<uint32_t> h_epoch_report;
    bool epoch_report_pending = false;
    uint32_t epoch_report_seq = 0;
    std::vector<uint32_t> epoch_report_channels;
    uint32_t wbfm_epochs_live = 0;          // channels with wbfm_epoch_left != 0
    std::vector<int32_t> rot_applied;       // [n_ch]: the rotation the device last ran with
    bool rot_changed = false;               // some channel's tails need rewriting (retail_kernel)
    DevArray<ScanConfig> d_scan_cfg;
    DevArray<ScanState> d_scan;
    DevArray<float> d_atan, d_fmlut;
    DevArray<float> d_half_lut;          // streaming WBFM kernel: |atan2| half table, tap matrices per rotation (-1, 0, +1)
    DevArray<uint32_t> d_amat[3];
    DevArray<uint32_t> d_amat4;          // FM tuner / AM-SSB stage 1 as MFMA operands: [fm: 3 rotations][am: 3 rotations][4][64][4]
    D4Args d4_args{};
    std::vector<float> fm_kmax;          // [n_ch]: like wbfm_kmax, for the FM chain
    bool stream_ok = false;              // the half table's symmetry holds on this host's libm
    std::vector<uint32_t> mode_gen, rot_gen;   // [n_ch]: bumped by iqd_set_mode / iqd_set_rotation (iqd_demod_accept restores only what nobody set meanwhile)
    std::vector<float> wbfm_kmax;        // [n_ch]: largest |K| a lead-in of the channel can still reach, or that was set since (casts stay bounded; iqd_accept.cpp: wbfm_gain_aged_out)
    // ... above this |K| it never falls back: 0.949^2048 = 3e-47 of K pi must lie below the 2^-100 under which the hand-off checks take
    // two de-emphasis states as agreeing (else a silent input would show the residue as state_repairs), and inf / NaN do not decay
    static constexpr float WBFM_KMAX_DECAYS = 1.0e15f;
    StreamArgs stream_args{};
    uint64_t stream_handoffs = 0;        // cold segments launched so far (their verification counts only mismatches)
    DevArray<uint32_t> d_counters;       // cumulative, read by iqd_get_stats
    DevArray<unsigned long long> d_stamps;
    PinnedArray<uint32_t> h_counters;

    // per-call scratch
    DevBuf stream_hist;   // boundary records of the streaming WBFM kernel, one StHist per segment
    DevBuf lists[FAM_COUNT + 1], mag_sums, blk_lists, vlen, records, base8k, base8k2, gain_trace, freq_trace, dc_records, dc_records2, repair_flags;
    size_t mag_sums_zero = 0;            // leading elements of mag_sums known to be zero (left so by the last squelch pass)
    // IQD_F_PREPASS_OVERLAP: a squelch-gated call's pre-pass (magnitudes of every block, decisions, open-block lists) runs on a
    // stream of its own, one call ahead of the pipelines: pre-pass(N + 1) overlaps chain(N).  Two sets of its buffers.
    Stream pre_stream;
    Event ev_pre_done[2], ev_chain_done[2], ev_main_decisions;
    DevBuf g_sums[2], g_blk[2], g_vlen[2];
    int gate_set = 0;
    bool chain_pending[2] = {false, false};   // ev_chain_done[set] has been recorded: the set's last reader may still run
    bool decisions_on_main = false;           // the last squelch decision pass ran on the main stream (ev_main_decisions)
    bool in_host_path = false;                // inside iqd_accept_iq: its staging copies are ordered on the main stream only
    DevBuf st_iq, st_pcm, st_count, st_mag, st_allowed;  // staging for host-pointer accepts
    // sliced host-pointer accepts: two staging sets, so that slice k+1 crosses PCIe while slice k runs
    DevBuf sl_iq[2], sl_pcm[2], sl_count[2], sl_mag[2], sl_allowed[2];
    Stream copy_stream;
    // mixed-mode calls: two side streams beside the engine's, so that the families' kernels share the GPU
    Stream fam_stream[3];               // side streams: with the engine's own, one lane per demodulator family
    Event fam_fork, fam_join[3];
    Event ev_in[2], ev_free[2];
    PinnedArray<uint32_t> h_slice_counts;   // [2][n_ch of a slice]
    DevArray<uint32_t> d_closed;            // squelch-gated calls: did any channel lose a block? (device word, pinned copy)
    PinnedArray<uint32_t> h_closed;
    PinnedArray<uint8_t> h_small;        // page-locked staging of small host-pointer calls: [input | pcm | counts | magnitudes | flags]

    bool profiling = false;
    // profiling: one event pair per timed launch, read back lazily so that accepts stay asynchronous
    std::vector<std::pair<Event, Event>> ev_free_pairs, ev_pending;
    iqd_stats stats{};
    std::string last_error;

    int fail(int code, const char *fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        last_error = buf;
        return code;
    }
};

#define HIP_TRY(e, call)                                                                          \
    do {                                                                                          \
        hipError_t err_ = (call);                                                                 \
        if (err_ != hipSuccess)                                                                   \
            return (e)->fail(IQD_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(err_),    \
                             __FILE__, __LINE__);                                                 \
    } while (0)

// the same, counting what is queued on the device (iqd_stats.device_launches / device_copies: launch_* calls and
// memcpy / memset operations; bench.py --config 0 reports them per block)
#define HIP_LAUNCH(e, call) do { (e)->stats.device_launches++; HIP_TRY(e, call); } while (0)
#define HIP_COPY(e, call) do { (e)->stats.device_copies++; HIP_TRY(e, call); } while (0)

static int family_of_mode(int mode)
{
    switch (mode) {
    case IQD_MODE_AM: return FAM_AM;
    case IQD_MODE_FM: return FAM_FM;
    case IQD_MODE_WBFM: return FAM_WBFM;
    case IQD_MODE_LSB: case IQD_MODE_USB: return FAM_SSB;
    default: return FAM_COUNT;
    }
}

static bool range_ok(const iqd_t *e, uint32_t first, uint32_t n)
{
    return e && n >= 1 && first < e->n_ch && n <= e->n_ch - first;
}

// A call is k whole blocks of block_bytes (k consecutive acceptIqData calls) - or ONE short block: the reference
// forwards whatever rtlsdr_read_sync returned (Radio.cc:1895-1906; DataConsumer.cc:238-242 only counts short
// reads) and acceptIqData averages the squelch over that call's samples (IqDataProcessor.cc:722-749).  A short
// block is a whole number of 64-byte units (32 samples: the period of the chains' /32 commutators; USB reads are
// multiples of 512 bytes) in every mode - the WBFM chain's 128-sample de-emphasis segments take a ragged head and tail
// since round 4 (iqd_wbfm.h: IirShape).  Returns the block size in force for the call, 0 if the length is not acceptable.
static uint32_t call_block_bytes(iqd_t *e, uint32_t first_ch, uint32_t n_ch, size_t bytes_per_ch)
{
    (void)first_ch;
    (void)n_ch;
    if (bytes_per_ch == 0) return 0;
    if (bytes_per_ch % e->block_bytes == 0) return e->block_bytes;
    if (bytes_per_ch >= e->block_bytes || bytes_per_ch % 64 != 0) return 0;
    return (uint32_t)bytes_per_ch;
}
#define IQD_LEN_MSG "bytes_per_ch (%zu) must be a positive multiple of block_bytes (%u), or one short block: a multiple of 64 below it"

namespace iqd {
// Uploads the channel parameters if they changed / the AGC configuration and the pending one-shot commands (iqd_engine.cpp).
// Call with e->mu held.
int upload_params(iqd_t *e);
int agc_sync(iqd_t *e);
}  // namespace iqd
