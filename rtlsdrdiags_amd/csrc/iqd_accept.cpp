// The accept path of libiqdemod.so (include/iqdemod.h: iqd_accept_iq_device, iqd_accept_iq) and the demodulators' own
// entry, which runs through it.
#include "iqd_engine_impl.h"

extern "C" {

// ---- accept: describe, plan, then queue ----------------------------------------------------------
// iqd_accept_iq_device() = prepare_call (parameter mirror, channel lists, under the lock) -> describe_call (the call as plain
// data) -> plan_call (iqd_plan.cpp: every tile / stream / one-launch / share decision, nothing queued yet; cached while the
// shape repeats) -> queue_prepass -> queue_family per family -> queue_commit.  The queue_* functions decide nothing.

static void rebuild_lists(iqd_t *e, uint32_t first_ch, uint32_t n_ch)
{
    for (auto &l : e->h_lists) l.clear();
    e->any_gated = e->any_agc = false;
    for (uint32_t c = 0; c < n_ch; c++) {
        const ChanParams &p = e->h_params[first_ch + c];
        e->h_lists[family_of_mode(p.mode)].push_back(c);
        ChanParams worst = p;   // a channel whose AGC runs (or ran) may sit at any gain up to the maximum
        if (e->agc_touched[first_ch + c] && worst.rx_gain_db < AGC_MAX_GAIN) worst.rx_gain_db = AGC_MAX_GAIN;
        if (!squelch_always_open(worst, e->consts)) e->any_gated = true;
        if (e->h_agc[first_ch + c].enabled) e->any_agc = true;
    }
    // Each family's channels in the order +Fs/4, no rotation, -Fs/4: the streaming kernels want the segments of one
    // rotation selector next to each other (a P wave's 16 segments share tap matrices); nothing else minds the order.
    for (int f = 0; f < FAM_COUNT; f++) {
        auto &l = e->h_lists[f];
        auto grp = [&](uint32_t c) { return 1 - e->h_params[first_ch + c].rotation; };
        std::stable_sort(l.begin(), l.end(), [&](uint32_t x, uint32_t y) { return grp(x) < grp(y); });
        for (int r = 0; r < 3; r++) e->rot_count[f][r] = 0;
        for (uint32_t c : l) e->rot_count[f][grp(c)]++;
    }
    e->list_first = first_ch;
    e->list_n = n_ch;
    e->lists_dirty = false;
}

namespace {
// What one accept call carries from phase to phase.
struct CallCtx {
    uint32_t first_ch = 0, n_ch = 0;
    const void *iq_dev = nullptr;
    size_t bytes_per_ch = 0;
    void *pcm_dev = nullptr, *pcm_count_dev = nullptr, *magnitude_dev = nullptr, *signal_present_dev = nullptr;
    uint32_t call_bb = 0, call_bs = 0, n_blocks = 0, vlen = 0;
    bool gated = false, any_agc = false, want_mag = false, pre_overlap = false, fused_mag = false;
    int pre_set = -1;                               // IQD_F_PREPASS_OVERLAP: the buffer set this call's pre-pass filled
    DevBuf *gate_blk = nullptr, *gate_vlen = nullptr;
    SquelchLaunch q{};
    ChainLaunch base{};
    const CallPlan *plan = nullptr;
    hipStream_t s_main = nullptr;
    bool lane_used[4] = {false, false, false, false};
    bool timed = false, evp_open = false;           // profiling: the event pair of the call
    std::pair<Event, Event> evp;
    MixedStreamArgs mix{};
    bool epoch_report_now = false;                  // this call's WBFM tail updates report whether a gain change is still in reach (h_epoch_report)
    ChainLaunch tail_a{};                           // a tail update (WBFM: repair check + state commit + tail) that rides in the squelch launch
    int tail_f = 0;
    bool tail_pending = false;
    bool tail_dc = false;                           // ... and the family's one-wave DC-removal pass with it (AM / SSB streaming launches)
};

int take_event_pair(iqd_t *e, CallCtx &x, hipStream_t s)
{
    if (e->ev_free_pairs.empty()) {
        Event a0, a1;
        HIP_TRY(e, hipEventCreate(a0.put()));
        HIP_TRY(e, hipEventCreate(a1.put()));
        e->ev_free_pairs.emplace_back(std::move(a0), std::move(a1));
    }
    x.evp = std::move(e->ev_free_pairs.back());
    e->ev_free_pairs.pop_back();
    HIP_TRY(e, hipEventRecord(x.evp.first, s));
    return IQD_OK;
}

// Channel c's last WBFM gain change has left its lead-ins' reach (wbfm_epoch_left went to 0): the chain has consumed TAIL
// samples with the current K, the de-emphasis (0.949 per sample) has taken whatever state the earlier gains left down by
// 3 10^-47, and the tile kernel's own rule (iqd_kernels.hip: wbfm_run_tile, K and the k_before in reach) sees the current K alone.
// So wbfm_kmax - which keeps a call off the bounded (int16) casts, the streaming pipeline and the one launch - falls back to the K
// the device runs with and the one a setter may have stored meanwhile; it used to stay at the largest K since creation, and
// ONE overlarge gain kept the channel's calls on the tile kernel for good.  It still does above WBFM_KMAX_DECAYS (iqd_engine_impl.h),
// and fm_kmax, which has no epoch mirror on the host to age it, never falls.  Call with e->mu held (iqd_set_gain raises wbfm_kmax
// under it).
void wbfm_gain_aged_out(iqd_t *e, uint32_t c)
{
    if (!(e->wbfm_kmax[c] < iqd_engine::WBFM_KMAX_DECAYS)) return;
    const float applied = fabsf(e->k_applied[2 * c]), pending = fabsf(e->h_params[c].wbfm_k);
    e->wbfm_kmax[c] = pending <= applied ? applied : pending;   // (a NaN just set: kept)
}
}  // namespace

// Under the lock: the epoch mirror's ageing report, parameter upload, channel lists, AGC configuration.
static int prepare_call(iqd_t *e, CallCtx &x)
{
    hipStream_t s = e->stream;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->epoch_report_pending && ((volatile uint32_t *)e->h_epoch_report)[1] == e->epoch_report_seq) {   // (see wbfm_epoch_seq)
        if (((volatile uint32_t *)e->h_epoch_report)[0] == 0u)
            for (uint32_t c : e->epoch_report_channels)
                if (e->wbfm_epoch_left[c] && e->wbfm_epoch_seq[c] <= e->epoch_report_seq) {
                    e->wbfm_epoch_left[c] = 0;
                    e->wbfm_epochs_live--;
                    wbfm_gain_aged_out(e, c);
                }
        e->epoch_report_pending = false;
    }
    {
        int rc = upload_params(e);
        if (rc != IQD_OK) return rc;
    }
    e->accept_seq++;
    if (e->lists_dirty || e->list_first != x.first_ch || e->list_n != x.n_ch) {
        rebuild_lists(e, x.first_ch, x.n_ch);
        for (int f = 0; f <= FAM_COUNT; f++) {
            const auto &l = e->h_lists[f];
            if (l.empty()) continue;
            HIP_TRY(e, e->lists[f].ensure(l.size() * sizeof(uint32_t)));
            HIP_COPY(e, hipMemcpyAsync(e->lists[f].p, l.data(), l.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        }
        HIP_TRY(e, hipStreamSynchronize(s));
    }
    int rc = agc_sync(e);
    if (rc != IQD_OK) return rc;
    x.gated = e->any_gated;
    x.any_agc = e->any_agc;
    return IQD_OK;
}

// The call as plain data for plan_call(): per family how many channels, per rotation selector, whether every gain keeps
// the (int16) casts bounded, whether a WBFM gain change is still in reach of a lead-in.
static void describe_call(const iqd_t *e, const CallCtx &x, CallShape &c)
{
    c = CallShape{};
    c.vlen = x.vlen;
    c.pcm_per_ch = (uint32_t)(x.bytes_per_ch / 64);
    c.gated = x.gated;
    for (int f = 0; f < FAM_COUNT; f++) {
        const auto &l = e->h_lists[f];
        FamilyShape &s = c.fam[f];
        s.n_list = (uint32_t)l.size();
        if (l.empty()) continue;
        for (int r = 0; r < 3; r++) s.rot_count[r] = e->rot_count[f][r];
        // (from the snapshot prepare_call took under the lock, not from the live parameters a setter may be writing: ADVICE r5.
        //  The list is sorted +Fs/4, none, -Fs/4, so its first channel's selector is the first non-empty group's)
        s.rot_first = s.rot_count[0] ? 1 : (s.rot_count[1] ? 0 : -1);
        if (f == FAM_WBFM)
            for (uint32_t ch : l) {
                s.cast_bounded = s.cast_bounded && e->wbfm_kmax[x.first_ch + ch] * 3.1730f < 2147483648.0f;
                s.epochs_in_reach = s.epochs_in_reach || (e->wbfm_epochs_live && e->wbfm_epoch_left[x.first_ch + ch] != 0);
            }
        if (f == FAM_FM)
            for (uint32_t ch : l) s.cast_bounded = s.cast_bounded && e->fm_kmax[x.first_ch + ch] * 6.35f < 2147483648.0f;
    }
}

static bool same_shape(const CallShape &a, const CallShape &b)
{
    if (a.vlen != b.vlen || a.pcm_per_ch != b.pcm_per_ch || a.gated != b.gated) return false;
    for (int f = 0; f < FAM_COUNT; f++) {
        const FamilyShape &p = a.fam[f], &q = b.fam[f];
        if (p.n_list != q.n_list || p.rot_count[0] != q.rot_count[0] || p.rot_count[1] != q.rot_count[1] || p.rot_count[2] != q.rot_count[2] ||
            p.rot_first != q.rot_first || p.cast_bounded != q.cast_bounded || p.epochs_in_reach != q.epochs_in_reach)
            return false;
    }
    return true;
}

// The squelch's part in front of the pipelines: the block sums start at zero; a gated call's magnitudes, decisions and
// open-block lists (inline on the engine's stream, or one call ahead on the pre-pass stream); the launch descriptor
// every family's launch starts from.
static int queue_prepass(iqd_t *e, CallCtx &x)
{
    hipStream_t s = x.s_main;
    const uint32_t n_ch = x.n_ch, n_blocks = x.n_blocks;
    // the pre-pass of a gated call one call ahead, on its own stream (include/iqdemod.h: IQD_F_PREPASS_OVERLAP)
    if (x.pre_overlap && !e->pre_stream) {
        HIP_TRY(e, hipStreamCreateWithFlags(e->pre_stream.put(), hipStreamNonBlocking));
        for (int k = 0; k < 2; k++) {
            HIP_TRY(e, hipEventCreateWithFlags(e->ev_pre_done[k].put(), hipEventDisableTiming));
            HIP_TRY(e, hipEventCreateWithFlags(e->ev_chain_done[k].put(), hipEventDisableTiming));
        }
        HIP_TRY(e, hipEventCreateWithFlags(e->ev_main_decisions.put(), hipEventDisableTiming));
        // whatever squelch pass ran before this one ran on the engine's stream, unrecorded: the new stream starts behind it
        HIP_TRY(e, hipEventRecord(e->ev_main_decisions, s));
        e->decisions_on_main = true;
    }
    if (!x.pre_overlap) {   // the sums start at zero: by memset, unless the previous call's squelch pass left this many of them zero
        const void *before = e->mag_sums.p;
        HIP_TRY(e, e->mag_sums.ensure((size_t)n_ch * n_blocks * sizeof(uint32_t)));
        if (e->mag_sums.p != before) e->mag_sums_zero = 0;
        if (x.want_mag && e->mag_sums_zero < (size_t)n_ch * n_blocks)
            HIP_COPY(e, hipMemsetAsync(e->mag_sums.p, 0, (size_t)n_ch * n_blocks * sizeof(uint32_t), s));
        e->mag_sums_zero = 0;   // from here on the call writes into them
    }

    SquelchLaunch &q = x.q;
    q.n_ch = n_ch; q.first_ch = x.first_ch; q.n_blocks = n_blocks; q.block_samples = x.call_bs;
    q.params = e->d_params;
    q.mag_sums = e->mag_sums.as<uint32_t>();
    q.tracker = e->d_tracker;
    q.magnitude = (uint32_t *)x.magnitude_dev;
    q.allowed = (uint8_t *)x.signal_present_dev;
    q.pcm_count = (uint32_t *)x.pcm_count_dev;
    q.agc_cfg = e->d_agc_cfg;
    q.agc = e->d_agc;
    q.any_agc = x.any_agc ? 1u : 0u;
    q.scan_cfg = e->d_scan_cfg;
    q.scan = e->d_scan;
    if (e->trace_on) {
        HIP_TRY(e, e->gain_trace.ensure((size_t)n_ch * n_blocks * sizeof(uint32_t)));
        q.gain_trace = e->gain_trace.as<uint32_t>();
        HIP_TRY(e, e->freq_trace.ensure((size_t)n_ch * n_blocks * sizeof(unsigned long long)));
        q.freq_trace = e->freq_trace.as<unsigned long long>();
        e->trace_first = x.first_ch; e->trace_n = n_ch; e->trace_blocks = n_blocks;
    }

    x.gate_blk = &e->blk_lists;
    x.gate_vlen = &e->vlen;
    if (x.pre_overlap) {
        // magnitudes, decisions and open-block lists of THIS call on the pre-pass stream, which the previous call's pipelines
        // (main stream) do not hold up: it waits for the decision pass before it (its own stream order - or the main stream's,
        // where the previous call's pass ran there), and for the last reader of the buffer set it is about to overwrite
        hipStream_t ps = e->pre_stream;
        x.pre_set = e->gate_set ^= 1;
        DevBuf &sums = e->g_sums[x.pre_set];
        x.gate_blk = &e->g_blk[x.pre_set];
        x.gate_vlen = &e->g_vlen[x.pre_set];
        if (e->chain_pending[x.pre_set]) HIP_TRY(e, hipStreamWaitEvent(ps, e->ev_chain_done[x.pre_set], 0));
        if (e->decisions_on_main) {
            HIP_TRY(e, hipStreamWaitEvent(ps, e->ev_main_decisions, 0));
            e->decisions_on_main = false;
        }
        HIP_TRY(e, sums.ensure((size_t)n_ch * n_blocks * sizeof(uint32_t)));
        HIP_TRY(e, x.gate_blk->ensure((size_t)n_ch * n_blocks * sizeof(uint32_t)));
        HIP_TRY(e, x.gate_vlen->ensure((size_t)n_ch * sizeof(uint32_t)));
        HIP_COPY(e, hipMemsetAsync(sums.p, 0, (size_t)n_ch * n_blocks * sizeof(uint32_t), ps));
        HIP_LAUNCH(e, launch_magnitude((const uint8_t *)x.iq_dev, x.bytes_per_ch, nullptr, n_ch, x.call_bs, n_blocks, sums.as<uint32_t>(), ps));
        q.mag_sums = sums.as<uint32_t>();
        q.blk_lists = x.gate_blk->as<uint32_t>();
        q.vlen_out = x.gate_vlen->as<uint32_t>();
        HIP_LAUNCH(e, launch_squelch(q, false, ps));
        HIP_TRY(e, hipEventRecord(e->ev_pre_done[x.pre_set], ps));
        HIP_TRY(e, hipStreamWaitEvent(s, e->ev_pre_done[x.pre_set], 0));   // the pipelines read the lists
    } else if (x.gated) {
        // pass 1: magnitudes of every block, then the squelch decisions and open-block lists
        if (e->pre_stream) HIP_TRY(e, hipStreamSynchronize(e->pre_stream));   // (a call of the overlapped kind before this one)
        HIP_TRY(e, e->blk_lists.ensure((size_t)n_ch * n_blocks * sizeof(uint32_t)));
        HIP_TRY(e, e->vlen.ensure((size_t)n_ch * sizeof(uint32_t)));
        HIP_LAUNCH(e, launch_magnitude((const uint8_t *)x.iq_dev, x.bytes_per_ch, nullptr, n_ch, x.call_bs, n_blocks, e->mag_sums.as<uint32_t>(), s));
        q.blk_lists = e->blk_lists.as<uint32_t>();
        q.vlen_out = e->vlen.as<uint32_t>();
        // (Round 2 read one word back here - did any channel lose a block? - to let an all-open call take the streaming
        // kernels, which could not gate.  They can now (a virtual sample axis over each channel's open blocks), so the
        // call stays asynchronous whatever the squelch decides.)
        HIP_LAUNCH(e, launch_squelch(q, false, s));
    }
    if (!x.gated && e->pre_stream) HIP_TRY(e, hipStreamWaitEvent(s, e->ev_pre_done[e->gate_set], 0));   // (the tracker / AGC state this call's squelch pass continues from)

    ChainLaunch &base = x.base;
    base.iq = (const uint8_t *)x.iq_dev;
    base.ch_stride_bytes = x.bytes_per_ch;
    base.first_ch = x.first_ch;
    base.vlen = x.vlen;
    base.vlen_gated = x.gated ? x.gate_vlen->as<uint32_t>() : nullptr;   // the chain kernels walk each channel's open blocks
    base.blk_lists = x.gated ? x.gate_blk->as<uint32_t>() : nullptr;
    base.n_blocks = n_blocks;
    base.block_samples = x.call_bs;
    base.block_magic = block_magic(x.call_bs);
    base.tails = e->d_tails;
    base.params = e->d_params;
    base.wbfm_carry = e->d_wcarry;
    base.dc_carry = e->d_dc;
    base.epochs = e->d_epochs;
    base.atan_lut = e->d_atan;
    base.fm_lut = e->d_fmlut;
    base.pcm = (int16_t *)x.pcm_dev;
    base.pcm_stride = x.bytes_per_ch / 64;
    base.mag_sums = e->mag_sums.as<uint32_t>();
    base.counters = e->d_counters;
    base.stamps = e->d_stamps;
    base.n_ch_call = n_ch;
    return IQD_OK;
}

// AM / SSB: the detector stream's buffer and the DC pass's records of this launch.  One buffer per family: short rows are
// written time-major by the tile kernels and channel-major by the streaming pipelines, and the two families of a call may
// take different paths (round 4's fuzzer: an AM family that streamed beside an SSB family on the tile kernels overwrote its
// detector stream).
static int attach_dc_buffers(iqd_t *e, CallCtx &x, int f, ChainLaunch &a, hipStream_t s)
{
    DevBuf &b8 = f == FAM_SSB ? e->base8k2 : e->base8k;
    HIP_TRY(e, b8.ensure((size_t)x.n_ch * x.base.pcm_stride * sizeof(int32_t)));
    a.base8k = b8.as<int32_t>();
    a.dc_tiles = (uint32_t)((x.base.pcm_stride + DC_TILE - 1) / DC_TILE);
    DevBuf &dcr = f == FAM_SSB ? e->dc_records2 : e->dc_records;   // AM and SSB may run side by side
    // records, then one redo flag per channel: zero between calls (dc_redo_kernel clears what it used)
    const size_t rec_bytes = (size_t)a.n_list * a.dc_tiles * sizeof(DcRecord);
    const bool grown = dcr.cap < rec_bytes + a.n_list * sizeof(uint32_t);
    HIP_TRY(e, dcr.ensure(rec_bytes + a.n_list * sizeof(uint32_t)));
    a.dc_records = dcr.p;
    // the flags sit behind the records, whose extent changes with the call: clear them whenever it may have
    // (same offset but more channels than last time: the new flags lie over old record bytes)
    size_t (&layout)[2] = e->dcr_layout[f == FAM_SSB];
    if (grown || layout[0] != rec_bytes || layout[1] < a.n_list) {
        HIP_COPY(e, hipMemsetAsync(dcr.as<char>() + rec_bytes, 0, a.n_list * sizeof(uint32_t), s));
        layout[0] = rec_bytes;
        layout[1] = a.n_list;
    }
    return IQD_OK;
}

// One family's launches as the plan says: its tile kernel or streaming pipeline (as a kernel of its own, or as a range of the
// one launch that queue_commit() starts), then what follows it - hand-off verification, repair, DC pass, tail update - unless
// that rides in the squelch launch at the call's end.
static int queue_family(iqd_t *e, CallCtx &x, int f)
{
    const CallPlan &plan = *x.plan;
    const FamilyPlan &fp = plan.fam[f];
    const bool fused = plan.fused, forked = plan.forked, streams = fp.path == PLAN_STREAM;
    const uint32_t n_list = (uint32_t)e->h_lists[f].size();
    hipStream_t s = fp.lane == 0 ? x.s_main : e->fam_stream[fp.lane - 1];
    if (fp.lane != 0 && !x.lane_used[fp.lane]) HIP_TRY(e, hipStreamWaitEvent(s, e->fam_fork, 0));
    x.lane_used[fp.lane] = true;

    ChainLaunch a = x.base;
    a.ch_list = e->lists[f].as<uint32_t>();
    a.n_list = n_list;
    a.tile_len = fp.tile_len;
    a.tiles_per_ch = fp.tiles_per_ch;
    if (f == FAM_WBFM && x.gated && e->wbfm_epochs_live && !e->epoch_report_pending) {
        bool any = false;
        for (uint32_t c : e->h_lists[FAM_WBFM]) any = any || e->wbfm_epoch_left[x.first_ch + c] != 0;
        if (any) {
            if (!e->h_epoch_report) HIP_TRY(e, e->h_epoch_report.alloc(2));
            ((volatile uint32_t *)e->h_epoch_report)[0] = 0u;
            a.epoch_report = e->h_epoch_report;
            e->epoch_report_channels.clear();
            for (uint32_t c : e->h_lists[FAM_WBFM]) e->epoch_report_channels.push_back(x.first_ch + c);
            x.epoch_report_now = true;
        }
    }
    if (e->profiling && !x.timed && !fused) {
        int rc = take_event_pair(e, x, s);
        if (rc != IQD_OK) return rc;
    }
    if (fused) {   // a range of the one launch's workgroups
        a.wg_first = fp.wg_first;
        a.wg_count = fp.grid;
    }
    if (f == FAM_WBFM) {
        HIP_TRY(e, e->records.ensure((size_t)n_list * a.tiles_per_ch * sizeof(WbfmRecord)));
        a.records = e->records.as<WbfmRecord>();
        if (e->repair_flags.cap < n_list * sizeof(uint32_t)) {   // zero between calls: the repair kernel clears what it used
            HIP_TRY(e, e->repair_flags.ensure(n_list * sizeof(uint32_t)));
            HIP_COPY(e, hipMemsetAsync(e->repair_flags.p, 0, e->repair_flags.cap, s));
        }
        a.repair_flags = e->repair_flags.as<uint32_t>();
        if (streams) {
            const int stream_rot = e->plan_shape.fam[FAM_WBFM].rot_first;   // (the plan's snapshot: queue_* decide nothing and read no live parameter)
            StreamArgs sa = e->stream_args;
            sa.amat = e->d_amat[stream_rot + 1];
            sa.half_lut = e->d_half_lut;
            sa.n_segments = n_list * a.tiles_per_ch;
            sa.grouped = fp.grouped ? 1u : 0u;
            for (int r = 0; r < 3; r++) {
                sa.group_start[r] = fp.grouped ? fp.group_start[r] : 0u;
                sa.group_li0[r] = fp.grouped ? fp.group_li0[r] : 0u;
                sa.group_nseg[r] = fp.grouped ? fp.group_nseg[r] : 0u;
                sa.amat3[r] = e->d_amat[2 - r];          // d_amat[] is indexed by selector + 1; the groups run +1, 0, -1
            }
            sa.group_start[3] = fp.grouped ? fp.group_start[3] : 0u;
            sa.rounds = fp.rounds;
            sa.rings = fp.rings;
            HIP_TRY(e, e->stream_hist.ensure((size_t)sa.n_segments * sizeof(StHist)));
            sa.hist = e->stream_hist.as<StHist>();
            a.verify_at_end = x.gated ? 2u : 1u;   // (2: the hand-offs are counted on the device - how many tiles a channel has depends on its squelch)
            if (fused) {   // the fix-up rides in the launch behind the one launch
                x.mix.a[f] = a;
                x.mix.sa = sa;
                x.mix.wbfm_rot = stream_rot;
            } else {
                HIP_LAUNCH(e, launch_wbfm_stream(a, sa, stream_rot, x.fused_mag, fp.epochs, fp.grid, s));
                HIP_LAUNCH(e, launch_wbfm_stream_fixup(a, sa, s));
            }
            if (!x.gated) e->stream_handoffs += (uint64_t)n_list * ((x.vlen + a.tile_len - 1) / a.tile_len - 1);
            e->stats.stream_launches++;
        } else {
            HIP_LAUNCH(e, launch_wbfm(a, x.gated, x.fused_mag, n_list * a.tiles_per_ch, s));
        }
    } else {
        D4Args d4 = e->d4_args;
        if (streams) {
            for (int r = 0; r < 3; r++) {
                d4.group_start[r] = fp.group_start[r];
                d4.group_li0[r] = fp.group_li0[r];
                d4.group_nseg[r] = fp.group_nseg[r];
            }
            d4.group_start[3] = fp.group_start[3];
            d4.amat = e->d_amat4 + (size_t)(f == FAM_FM ? 0 : 3) * 4 * 64 * 4;
            d4.fm_lut = e->d_fmlut;
            d4.halo = (int32_t)fp.halo;
            d4.lead_shift = fp.lead_shift;
            d4.rounds = fp.rounds;
            d4.rings = fp.rings;
        }
        if (f != FAM_FM) {
            int rc = attach_dc_buffers(e, x, f, a, s);
            if (rc != IQD_OK) return rc;
            if (streams) {   // (the pipeline writes the detector stream channel-major)
                a.base_stride_ch = x.base.pcm_stride;
                a.base_stride_t = 1;
                // ... as int16 into the PCM rows themselves when the DC pass behind it is the one-wave pass (in place, round 6);
                // rows so long that they take the many-wave pass keep the int32 stream: its tiles warm up over their neighbours' input
                static const bool no_det16 = getenv("IQD_NO_DET16") != nullptr;   // (the A/B)
                a.det16 = a.dc_tiles < 2 && !no_det16 ? 1u : 0u;
            }
        }
        if (streams) {
            if (fused) {
                x.mix.a[f] = a;
                x.mix.d4[f] = d4;
            } else {
                HIP_LAUNCH(e, launch_d4_stream(a, d4, f == FAM_FM ? D4_FM : f == FAM_AM ? D4_AM : D4_SSB, x.fused_mag, fp.grid, s));
                // the DC-removal pass: a role of the call's closing launch where there is one to ride in and the rows take the
                // one-wave pass (round 5: 0.019 ms and a queue gap less per step); else its own launches
                x.tail_dc = f != FAM_FM && a.dc_tiles < 2 && !forked && !x.gated && !e->demod_bypass &&
                            (x.want_mag || x.pcm_count_dev || x.signal_present_dev || e->trace_on);
                if (f != FAM_FM && !x.tail_dc) HIP_LAUNCH(e, launch_am_dc(a, f, s, true));
            }
            e->stats.stream_launches++;
        } else if (f == FAM_FM) {
            HIP_LAUNCH(e, launch_fm(a, x.gated, x.fused_mag, n_list * a.tiles_per_ch, s));
        } else {
            HIP_LAUNCH(e, launch_am(a, f, x.gated, x.fused_mag, n_list * a.tiles_per_ch, s));
        }
    }
    if (e->profiling && !x.timed && !fused) {
        // the pair closes behind the step's last launch (queue_commit), so that the timed region holds EVERY launch of the step
        // (the repair-check / commit / squelch launch was left out)
        x.evp_open = true;   // (forked plans opened theirs in front of the fork: iqd_accept_iq_device)
        x.timed = true;
    }
    e->stats.kernel_launches++;
    if (fused) return IQD_OK;   // (one launch for all the families and one for what follows them: queue_commit)
    if (f == FAM_WBFM && !x.gated && e->wbfm_epochs_live) {   // every channel of the family has consumed vlen samples
        std::lock_guard<std::mutex> lk(e->mu);
        for (uint32_t c : e->h_lists[FAM_WBFM]) {
            uint32_t &left = e->wbfm_epoch_left[x.first_ch + c];
            if (!left) continue;
            left = left > x.vlen ? left - x.vlen : 0u;
            if (!left) {
                e->wbfm_epochs_live--;
                wbfm_gain_aged_out(e, x.first_ch + c);
            }
        }
    }
    const bool rides_with_squelch = !forked && !x.gated && !e->demod_bypass &&
                                    (x.want_mag || x.pcm_count_dev || x.signal_present_dev || e->trace_on);
    if (f == FAM_WBFM) {
        // hand-off verification (streaming launches: done by their fix-up kernel), repair of what it flags
        // (normally an immediate exit), then state commit + tail - in the squelch launch at the call's end when the call has
        // no other family
        if (!streams) HIP_LAUNCH(e, launch_wbfm_verify(a, s));
        if (rides_with_squelch) {
            x.tail_a = a;
            x.tail_f = f;
            x.tail_pending = true;
        } else {
            HIP_LAUNCH(e, launch_wbfm_repair(a, x.gated, s));   // (ends with the channels' state commit and tail update)
        }
    } else if (rides_with_squelch) {
        x.tail_a = a;        // the only family of the call: its tail update rides in the squelch launch
        x.tail_f = f;
        x.tail_pending = true;
    } else {
        HIP_LAUNCH(e, launch_tail_update(a, f, s));
    }
    return IQD_OK;
}

// Behind the families: the one launch that holds all of them (fused plans) and its follower, the side streams' join, the
// magnitudes of channels in mode None, the squelch pass with whatever rides in it, the call's events and counters.
static int queue_commit(iqd_t *e, CallCtx &x)
{
    const CallPlan &plan = *x.plan;
    hipStream_t s = x.s_main;
    if (plan.fused) {
        if (e->profiling) {
            int rc = take_event_pair(e, x, s);
            if (rc != IQD_OK) return rc;
        }
        HIP_LAUNCH(e, launch_mixed_stream(x.mix, x.fused_mag, x.gated, plan.mix_wgs, s));
        e->stats.mixed_launches++;
        MixedTailArgs mt{};
        for (int f = 0; f < FAM_COUNT; f++) mt.a[f] = x.mix.a[f];
        mt.sa = x.mix.sa;
        HIP_LAUNCH(e, launch_mixed_tail(mt, s));
        if (e->profiling) x.evp_open = true;   // (the timed region: the pipelines AND every follower - fix-up, DC passes, tails, the squelch launch)
        if (x.mix.a[FAM_WBFM].wg_count) {   // repair check, state commit and tail of the WBFM channels: in the squelch launch below
            x.tail_a = x.mix.a[FAM_WBFM];
            x.tail_f = FAM_WBFM;
            x.tail_pending = true;
        }
        // (the WBFM family's epoch mirror: a fused plan has no gain change in reach, nothing to age)
    }
    for (int k = 1; k < 4; k++)
        if (x.lane_used[k]) {
            HIP_TRY(e, hipEventRecord(e->fam_join[k - 1], e->fam_stream[k - 1]));
            HIP_TRY(e, hipStreamWaitEvent(s, e->fam_join[k - 1], 0));
        }

    // channels in mode None still report their magnitudes
    if (x.fused_mag && !e->h_lists[FAM_COUNT].empty())
        HIP_LAUNCH(e, launch_magnitude((const uint8_t *)x.iq_dev, x.bytes_per_ch, e->lists[FAM_COUNT].as<uint32_t>(),
                                    (uint32_t)e->h_lists[FAM_COUNT].size(), x.call_bs, x.n_blocks, e->mag_sums.as<uint32_t>(), s));
    if (!x.gated && !e->demod_bypass && (x.want_mag || x.pcm_count_dev || x.signal_present_dev || e->trace_on)) {
        x.q.zero_sums_after = x.any_agc ? 0u : 1u;   // (a running AGC reads them again in the tracking pass)
        HIP_LAUNCH(e, launch_squelch(x.q, true, s, x.tail_pending ? &x.tail_a : nullptr, x.tail_f, x.tail_pending && x.tail_dc));
        x.tail_pending = false;
        if (x.q.zero_sums_after) e->mag_sums_zero = (size_t)x.n_ch * x.n_blocks;
    }
    if (x.tail_pending) {   // (no squelch launch to ride in)
        if (x.tail_f == FAM_WBFM) HIP_LAUNCH(e, launch_wbfm_repair(x.tail_a, x.gated, s));
        else HIP_LAUNCH(e, launch_tail_update(x.tail_a, x.tail_f, s));
    }

    if (x.evp_open) {
        HIP_TRY(e, hipEventRecord(x.evp.second, s));
        e->ev_pending.push_back(std::move(x.evp));
    }
    if (x.pre_set >= 0) {   // this call's pipelines are the last readers of its buffer set
        HIP_TRY(e, hipEventRecord(e->ev_chain_done[x.pre_set], s));
        e->chain_pending[x.pre_set] = true;
    } else if (e->pre_stream && !e->demod_bypass) {
        // a squelch pass on the main stream - this call's closing pass, or a gated call's inline decisions (those left
        // no event behind) - : the next pre-pass continues from it
        HIP_TRY(e, hipEventRecord(e->ev_main_decisions, s));
        e->decisions_on_main = true;
    }
    if (x.epoch_report_now) {   // behind everything this call queued (the side streams have joined)
        HIP_LAUNCH(e, launch_write_word(e->h_epoch_report + 1, e->accept_seq, s));
        e->epoch_report_pending = true;
        e->epoch_report_seq = e->accept_seq;
    }
    e->stats.accepts++;
    e->stats.samples += (uint64_t)x.vlen * x.n_ch;
    return IQD_OK;
}

int iqd_accept_iq_device(iqd_t *e, uint32_t first_ch, uint32_t n_ch, const void *iq_dev, size_t bytes_per_ch,
                         void *pcm_dev, void *pcm_count_dev, void *magnitude_dev, void *signal_present_dev)
{
    if (!range_ok(e, first_ch, n_ch) || !iq_dev || !pcm_dev) return e ? e->fail(IQD_EINVAL, "bad channel range or NULL buffer") : IQD_EINVAL;
    const uint32_t call_bb = call_block_bytes(e, first_ch, n_ch, bytes_per_ch);
    if (!call_bb) return e->fail(IQD_EINVAL, IQD_LEN_MSG, bytes_per_ch, e->block_bytes);
    if (bytes_per_ch / 2 > 0x7fff0000ull) return e->fail(IQD_EINVAL, "bytes_per_ch too large");
    if (((uintptr_t)iq_dev & 15) != 0) return e->fail(IQD_EINVAL, "iq_dev must be 16-byte aligned");
    (void)hipSetDevice(e->device);

    CallCtx x;
    x.first_ch = first_ch; x.n_ch = n_ch; x.iq_dev = iq_dev; x.bytes_per_ch = bytes_per_ch;
    x.pcm_dev = pcm_dev; x.pcm_count_dev = pcm_count_dev; x.magnitude_dev = magnitude_dev; x.signal_present_dev = signal_present_dev;
    x.call_bb = call_bb;
    x.call_bs = call_bb / 2;
    x.n_blocks = (uint32_t)(bytes_per_ch / call_bb);
    x.vlen = (uint32_t)(bytes_per_ch / 2);
    x.s_main = e->stream;
    int rc = prepare_call(e, x);
    if (rc != IQD_OK) return rc;
    if (e->demod_bypass) {   // {Am,Fm,WbFm,Ssb}Demodulator::acceptIqData: nothing of the processor's squelch path runs or moves
        x.gated = x.any_agc = false;
        x.pcm_count_dev = x.magnitude_dev = x.signal_present_dev = nullptr;
    }
    x.want_mag = !e->demod_bypass && (x.gated || x.any_agc || !(e->flags & IQD_F_NO_MAGNITUDE) || x.magnitude_dev);
    x.pre_overlap = x.gated && (e->flags & IQD_F_PREPASS_OVERLAP) && !e->trace_on && !e->in_host_path;
    x.fused_mag = x.want_mag && !x.gated;

    // the plan: decided before anything of the call is queued, kept while the call's shape repeats
    CallShape shape;
    describe_call(e, x, shape);
    if (!e->plan_valid || !same_shape(shape, e->plan_shape)) {
        plan_call(e->knobs, shape, e->plan);
        e->plan_shape = shape;
        e->plan_valid = true;
    }
    x.plan = &e->plan;
    const CallPlan &plan = e->plan;

    rc = queue_prepass(e, x);
    if (rc != IQD_OK) return rc;
    if (plan.forked) {
        if (!e->fam_fork) {
            int lo = 0, hi = 0;   // numerically lower = higher priority
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            HIP_TRY(e, hipEventCreateWithFlags(e->fam_fork.put(), hipEventDisableTiming));
            for (int k = 0; k < 3; k++) {
                HIP_TRY(e, hipStreamCreateWithPriority(e->fam_stream[k].put(), hipStreamNonBlocking, k == 0 ? hi : lo));
                HIP_TRY(e, hipEventCreateWithFlags(e->fam_join[k].put(), hipEventDisableTiming));
            }
        }
        // the detector-stream buffers before the fork (an allocation that grows one must not free what a side stream still reads)
        if (!e->h_lists[FAM_AM].empty()) HIP_TRY(e, e->base8k.ensure((size_t)n_ch * x.base.pcm_stride * sizeof(int32_t)));
        if (!e->h_lists[FAM_SSB].empty()) HIP_TRY(e, e->base8k2.ensure((size_t)n_ch * x.base.pcm_stride * sizeof(int32_t)));
        // several families as kernels of their own on side streams: the timed region opens in front of the fork and closes behind
        // the join and the closing launch (queue_commit), like every other arrangement's - every launch of the step (ADVICE r5:
        // it used to hold the first family's launches only, so kernel_ms was not comparable across arrangements)
        if (!plan.fused && e->profiling) {
            rc = take_event_pair(e, x, x.s_main);
            if (rc != IQD_OK) return rc;
            x.timed = true;
            x.evp_open = true;
        }
        if (!plan.fused) HIP_TRY(e, hipEventRecord(e->fam_fork, x.s_main));
    }
    for (int oi = 0; oi < FAM_COUNT; oi++) {
        const int f = plan.order[oi];
        if (!plan.fam[f].present) continue;
        rc = queue_family(e, x, f);
        if (rc != IQD_OK) return rc;
    }
    return queue_commit(e, x);
}

// Large host-pointer accepts are cut into slices of about SLICE_BYTES that go through two sets of device
// staging buffers: the upload of slice k+1 (copy stream) overlaps the kernels and the download of slice k
// (engine stream).  A slice is either a time range of every channel of the call (few long rows) or a range of
// whole rows (many channels).  Per-channel state is carried from slice to slice exactly as from one accept call
// to the next, so the result equals the unsliced call; squelch-gated rows are compacted on the host at the end.
static const size_t SLICE_BYTES = (size_t)32 << 20;
static const size_t SMALL_CALL_BYTES = (size_t)256 << 10;   // host-pointer calls up to this size run straight out of page-locked host memory

static int accept_sliced(iqd_t *e, uint32_t first_ch, uint32_t n_ch, const uint8_t *iq, size_t bytes_per_ch, uint32_t call_bb,
                         int16_t *pcm, uint32_t *pcm_count, uint32_t *magnitude, uint8_t *signal_present)
{
    hipStream_t s = e->stream;
    if (!e->copy_stream) {
        HIP_TRY(e, hipStreamCreateWithFlags(e->copy_stream.put(), hipStreamNonBlocking));
        for (int b = 0; b < 2; b++) {
            HIP_TRY(e, hipEventCreateWithFlags(e->ev_in[b].put(), hipEventDisableTiming));
            HIP_TRY(e, hipEventCreateWithFlags(e->ev_free[b].put(), hipEventDisableTiming));
        }
    }
    const size_t bb = call_bb;   // the block size in force for THIS call: one short block has bb = bytes_per_ch
    const size_t row_blocks = bytes_per_ch / bb;
    // slice shape: sc channels x st bytes of each row
    size_t sc, st;
    if ((size_t)n_ch * bb <= SLICE_BYTES && row_blocks > 1) {   // time slices of all channels
        sc = n_ch;
        st = std::max<size_t>(1, SLICE_BYTES / ((size_t)n_ch * bb)) * bb;
        if (st > bytes_per_ch) st = bytes_per_ch;
    } else {                                                    // ranges of whole rows
        st = bytes_per_ch;
        sc = std::max<size_t>(1, SLICE_BYTES / bytes_per_ch);
        if (sc > n_ch) sc = n_ch;
    }
    const size_t n_tslices = (bytes_per_ch + st - 1) / st, n_cslices = (n_ch + sc - 1) / sc;
    const size_t n_slices = n_tslices * n_cslices;
    const size_t st_blocks = st / bb;
    if (e->h_slice_counts.n < 2 * sc) HIP_TRY(e, e->h_slice_counts.alloc(2 * sc));
    for (int b = 0; b < 2; b++) {
        HIP_TRY(e, e->sl_iq[b].ensure(sc * st));
        HIP_TRY(e, e->sl_pcm[b].ensure(sc * (st / 64) * sizeof(int16_t)));
        HIP_TRY(e, e->sl_count[b].ensure(sc * sizeof(uint32_t)));
        HIP_TRY(e, e->sl_mag[b].ensure(sc * st_blocks * sizeof(uint32_t)));
        HIP_TRY(e, e->sl_allowed[b].ensure(sc * st_blocks));
    }
    std::vector<uint32_t> filled(n_ch, 0);   // PCM samples already in place at the front of each row
    const size_t row_pcm = bytes_per_ch / 64;

    struct Slice { size_t c0, nc, t0, tb; };
    auto slice_at = [&](size_t k) {
        Slice x;
        const size_t ci = k / n_tslices, ti = k % n_tslices;
        x.c0 = ci * sc; x.nc = std::min(sc, (size_t)n_ch - x.c0);
        x.t0 = ti * st; x.tb = std::min(st, bytes_per_ch - x.t0);
        return x;
    };
    auto upload = [&](size_t k) -> int {
        const Slice x = slice_at(k);
        const int b = (int)(k & 1);
        if (k >= 2) HIP_TRY(e, hipStreamWaitEvent(e->copy_stream, e->ev_free[b], 0));
        HIP_COPY(e, hipMemcpy2DAsync(e->sl_iq[b].p, x.tb, iq + x.c0 * bytes_per_ch + x.t0, bytes_per_ch, x.tb, x.nc,
                                    hipMemcpyHostToDevice, e->copy_stream));
        HIP_TRY(e, hipEventRecord(e->ev_in[b], e->copy_stream));
        return IQD_OK;
    };
    // what slice k-1 left in the pinned count buffer: compact its PCM behind what the rows already hold
    auto settle = [&](size_t k) {
        const Slice x = slice_at(k);
        const uint32_t *cnt = e->h_slice_counts + (k & 1) * sc;
        for (size_t c = 0; c < x.nc; c++) {
            int16_t *row = pcm + (x.c0 + c) * row_pcm;
            uint32_t &have = filled[x.c0 + c];
            const size_t landed = x.t0 / 64;
            if (cnt[c] && have != landed) memmove(row + have, row + landed, cnt[c] * sizeof(int16_t));
            have += cnt[c];
        }
    };

    int rc = upload(0);
    if (rc != IQD_OK) return rc;
    for (size_t k = 0; k < n_slices; k++) {
        const Slice x = slice_at(k);
        const int b = (int)(k & 1);
        if (k + 1 < n_slices && (rc = upload(k + 1)) != IQD_OK) return rc;
        HIP_TRY(e, hipStreamWaitEvent(s, e->ev_in[b], 0));
        HIP_COPY(e, hipMemsetAsync(e->sl_pcm[b].p, 0, x.nc * (x.tb / 64) * sizeof(int16_t), s));
        rc = iqd_accept_iq_device(e, first_ch + (uint32_t)x.c0, (uint32_t)x.nc, e->sl_iq[b].p, x.tb, e->sl_pcm[b].p,
                                  e->sl_count[b].p, magnitude ? e->sl_mag[b].p : nullptr,
                                  signal_present ? e->sl_allowed[b].p : nullptr);
        if (rc != IQD_OK) return rc;
        if (e->demod_bypass)   // (no squelch pass, nothing dropped: every row of the slice is full)
            HIP_COPY(e, hipMemsetD32Async((hipDeviceptr_t)e->sl_count[b].p, (int)(x.tb / 64), x.nc, s));
        if (k >= 1) {   // the previous slice's downloads are complete once its count copy is
            HIP_TRY(e, hipEventSynchronize(e->ev_free[b ^ 1]));
            settle(k - 1);
        }
        const size_t tpcm = x.tb / 64, tblk = x.tb / bb;
        HIP_COPY(e, hipMemcpy2DAsync(pcm + x.c0 * row_pcm + x.t0 / 64, row_pcm * sizeof(int16_t), e->sl_pcm[b].p,
                                    tpcm * sizeof(int16_t), tpcm * sizeof(int16_t), x.nc, hipMemcpyDeviceToHost, s));
        if (magnitude)
            HIP_COPY(e, hipMemcpy2DAsync(magnitude + x.c0 * row_blocks + x.t0 / bb, row_blocks * sizeof(uint32_t),
                                        e->sl_mag[b].p, tblk * sizeof(uint32_t), tblk * sizeof(uint32_t), x.nc,
                                        hipMemcpyDeviceToHost, s));
        if (signal_present)
            HIP_COPY(e, hipMemcpy2DAsync(signal_present + x.c0 * row_blocks + x.t0 / bb, row_blocks, e->sl_allowed[b].p,
                                        tblk, tblk, x.nc, hipMemcpyDeviceToHost, s));
        HIP_COPY(e, hipMemcpyAsync(e->h_slice_counts + b * sc, e->sl_count[b].p, x.nc * sizeof(uint32_t),
                                  hipMemcpyDeviceToHost, s));
        HIP_TRY(e, hipEventRecord(e->ev_free[b], s));
    }
    HIP_TRY(e, hipStreamSynchronize(s));
    settle(n_slices - 1);
    for (uint32_t c = 0; c < n_ch; c++)   // like the unsliced path: zeros behind the valid samples
        if (filled[c] < row_pcm) memset(pcm + c * row_pcm + filled[c], 0, (row_pcm - filled[c]) * sizeof(int16_t));
    if (pcm_count) memcpy(pcm_count, filled.data(), n_ch * sizeof(uint32_t));
    return IQD_OK;
}

int iqd_accept_iq(iqd_t *e, uint32_t first_ch, uint32_t n_ch, const uint8_t *iq, size_t bytes_per_ch,
                  int16_t *pcm, uint32_t *pcm_count, uint32_t *magnitude, uint8_t *signal_present)
{
    if (!range_ok(e, first_ch, n_ch) || !iq || !pcm) return e ? e->fail(IQD_EINVAL, "bad channel range or NULL buffer") : IQD_EINVAL;
    const uint32_t call_bb = call_block_bytes(e, first_ch, n_ch, bytes_per_ch);
    if (!call_bb) return e->fail(IQD_EINVAL, IQD_LEN_MSG, bytes_per_ch, e->block_bytes);
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    struct HostPath { iqd_t *e; HostPath(iqd_t *e_) : e(e_) { e->in_host_path = true; } ~HostPath() { e->in_host_path = false; } } host_path(e);
    const size_t in_bytes = (size_t)n_ch * bytes_per_ch;
    const size_t pcm_bytes = (size_t)n_ch * (bytes_per_ch / 64) * sizeof(int16_t);
    const size_t nb = (size_t)n_ch * (bytes_per_ch / call_bb);
    if (in_bytes >= 2 * SLICE_BYTES)
        return accept_sliced(e, first_ch, n_ch, iq, bytes_per_ch, call_bb, pcm, pcm_count, magnitude, signal_present);
    if (in_bytes <= SMALL_CALL_BYTES) {
        // A small call - the reference's own operating point is ONE 32768-byte block per call (DataConsumer.cc:333-346) -
        // is all latency: through the staging path it was an upload, two fills, two kernels and up to four downloads,
        // ~90 us per block.  Here the kernels read the block from, and write their results to, page-locked host memory
        // that the device addresses directly: no copy operation is queued at all, two launches and one wait remain.
        const size_t off_cnt = (pcm_bytes + 15) & ~(size_t)15, off_mag = off_cnt + (((size_t)n_ch * 4 + 15) & ~(size_t)15);
        const size_t off_al = off_mag + ((nb * 4 + 15) & ~(size_t)15), out_bytes = off_al + ((nb + 15) & ~(size_t)15);
        if (e->h_small.n < in_bytes + out_bytes + 16) HIP_TRY(e, e->h_small.alloc(2 * (in_bytes + out_bytes) + 4096));
        uint8_t *h_in = e->h_small, *h_out = e->h_small + ((in_bytes + 15) & ~(size_t)15);
        memcpy(h_in, iq, in_bytes);
        memset(h_out, 0, pcm_bytes);   // (zeros behind the valid samples, as the staging path leaves them)
        int rc = iqd_accept_iq_device(e, first_ch, n_ch, h_in, bytes_per_ch, h_out, h_out + off_cnt,
                                      magnitude ? h_out + off_mag : nullptr, signal_present ? h_out + off_al : nullptr);
        if (rc != IQD_OK) return rc;
        HIP_TRY(e, hipStreamSynchronize(s));
        memcpy(pcm, h_out, pcm_bytes);
        if (pcm_count) memcpy(pcm_count, h_out + off_cnt, (size_t)n_ch * sizeof(uint32_t));
        if (magnitude) memcpy(magnitude, h_out + off_mag, nb * sizeof(uint32_t));
        if (signal_present) memcpy(signal_present, h_out + off_al, nb);
        return IQD_OK;
    }
    HIP_TRY(e, e->st_iq.ensure(in_bytes));
    HIP_TRY(e, e->st_pcm.ensure(pcm_bytes));
    HIP_TRY(e, e->st_count.ensure(n_ch * sizeof(uint32_t)));
    HIP_TRY(e, e->st_mag.ensure(nb * sizeof(uint32_t)));
    HIP_TRY(e, e->st_allowed.ensure(nb));
    HIP_COPY(e, hipMemcpyAsync(e->st_iq.p, iq, in_bytes, hipMemcpyHostToDevice, s));
    HIP_COPY(e, hipMemsetAsync(e->st_pcm.p, 0, pcm_bytes, s));
    int rc = iqd_accept_iq_device(e, first_ch, n_ch, e->st_iq.p, bytes_per_ch, e->st_pcm.p, e->st_count.p,
                                  magnitude ? e->st_mag.p : nullptr, signal_present ? e->st_allowed.p : nullptr);
    if (rc != IQD_OK) return rc;
    HIP_COPY(e, hipMemcpyAsync(pcm, e->st_pcm.p, pcm_bytes, hipMemcpyDeviceToHost, s));
    if (pcm_count) HIP_COPY(e, hipMemcpyAsync(pcm_count, e->st_count.p, n_ch * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (magnitude) HIP_COPY(e, hipMemcpyAsync(magnitude, e->st_mag.p, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (signal_present) HIP_COPY(e, hipMemcpyAsync(signal_present, e->st_allowed.p, nb, hipMemcpyDeviceToHost, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    return IQD_OK;
}

// ---- the demodulators' own entry ----------------------------------------------------------------
// {Am,Fm,WbFm,Ssb}Demodulator::acceptIqData(int8_t *bufferPtr, uint32_t bufferLength), e.g. WbFmDemodulator.cc:383-411:
// SIGNED bytes as the processor hands them over (after the -128 and the rotation), straight into the demodulator -
// no squelch, no notification, no AGC.  The demodulator objects are the ones the processor uses (Radio.cc:150-181), so
// its filter state is shared with iqd_accept_iq of the same channel.  Run here as an accept of the same channel with
// the front end neutralised: offset-binary bytes s ^ 0x80, rotation selector 0 (a channel's kept tail is stored as raw
// bytes under its selector; retail_kernel rewrites it exactly when the selector moves, and back afterwards), the
// squelch path bypassed.
int iqd_demod_set_sideband(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int lsb)
{
    if (!range_ok(e, first_ch, n_ch)) return IQD_EINVAL;
    std::lock_guard<std::mutex> lk(e->mu);
    for (uint32_t c = first_ch; c < first_ch + n_ch; c++) {
        ChanParams &p = e->h_params[c];
        p.ssb_lsb = lsb ? 1 : 0;
        if (p.mode == IQD_MODE_LSB || p.mode == IQD_MODE_USB) p.mode = lsb ? IQD_MODE_LSB : IQD_MODE_USB;   // (one flag in the reference: SsbDemodulator.cc:333-367)
    }
    e->params_dirty = e->lists_dirty = true;
    return IQD_OK;
}

int iqd_demod_accept(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int demod, const int8_t *iq, size_t bytes_per_ch, int16_t *pcm)
{
    if (!range_ok(e, first_ch, n_ch) || !iq || !pcm) return e ? e->fail(IQD_EINVAL, "bad channel range or NULL buffer") : IQD_EINVAL;
    if (demod < IQD_DEMOD_AM || demod > IQD_DEMOD_SSB) return e->fail(IQD_EINVAL, "demod must be IQD_DEMOD_AM .. IQD_DEMOD_SSB");
    if (bytes_per_ch == 0 || bytes_per_ch % 64 != 0)
        return e->fail(IQD_EINVAL, "bytes_per_ch (%zu) must be a positive multiple of 64", bytes_per_ch);
    // The channels as this call needs them; what the caller had set comes back afterwards.  A channel that already is in the
    // wanted mode with selector 0 is left alone: a bare demodulator object driven call after call (demod.cc, one block per
    // call) then costs no parameter upload, no list rebuild and no tail rewrite at all.
    std::vector<int32_t> mode0(n_ch), rot0(n_ch), mode1(n_ch);
    std::vector<uint32_t> mgen(n_ch), rgen(n_ch);   // the setters' generation counters as this call found them
    bool touched = false;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        if (e->mode_gen.size() < e->h_params.size()) e->mode_gen.resize(e->h_params.size(), 0u);
        if (e->rot_gen.size() < e->h_params.size()) e->rot_gen.resize(e->h_params.size(), 0u);
        for (uint32_t c = 0; c < n_ch; c++) {
            mgen[c] = e->mode_gen[first_ch + c];
            rgen[c] = e->rot_gen[first_ch + c];
            ChanParams &p = e->h_params[first_ch + c];
            mode0[c] = p.mode;
            rot0[c] = p.rotation;
            mode1[c] = demod == IQD_DEMOD_AM ? IQD_MODE_AM : demod == IQD_DEMOD_FM ? IQD_MODE_FM : demod == IQD_DEMOD_WBFM ? IQD_MODE_WBFM
                                             : (p.ssb_lsb ? IQD_MODE_LSB : IQD_MODE_USB);
            touched = touched || p.mode != mode1[c] || p.rotation != 0;
            p.mode = mode1[c];
            p.rotation = 0;
        }
        if (touched) e->params_dirty = e->lists_dirty = true;
    }
    e->demod_bypass = true;
    int rc = IQD_OK;
    // whole blocks first, then what is left as one short block; at most ~16 MiB of input per accept (the staging path)
    const size_t bb = e->block_bytes, row_pcm = bytes_per_ch / 64;
    size_t max_t = ((size_t)16 << 20) / n_ch / bb * bb;
    if (max_t < bb) max_t = bb;
    std::vector<uint8_t> u8;
    std::vector<int16_t> part;
    for (size_t t0 = 0; t0 < bytes_per_ch && rc == IQD_OK;) {
        const size_t rest = bytes_per_ch - t0;
        const size_t t = rest >= bb ? std::min(rest / bb * bb, max_t) : rest;
        u8.resize((size_t)n_ch * t);
        part.resize((size_t)n_ch * (t / 64));
        for (uint32_t c = 0; c < n_ch; c++) {
            const uint8_t *src = (const uint8_t *)iq + (size_t)c * bytes_per_ch + t0;
            uint8_t *dst = u8.data() + (size_t)c * t;
            for (size_t k = 0; k < t; k++) dst[k] = src[k] ^ 0x80u;
        }
        rc = iqd_accept_iq(e, first_ch, n_ch, u8.data(), t, part.data(), nullptr, nullptr, nullptr);
        if (rc == IQD_OK)
            for (uint32_t c = 0; c < n_ch; c++)
                memcpy(pcm + (size_t)c * row_pcm + t0 / 64, part.data() + (size_t)c * (t / 64), (t / 64) * sizeof(int16_t));
        t0 += t;
    }
    e->demod_bypass = false;
    if (touched) {
        // only what this call wrote and no setter has written since - by the setters' generation counters, not by value: a
        // set_mode to the demodulator's own mode or a set_rotation(0) issued during the call keeps its value too
        std::lock_guard<std::mutex> lk(e->mu);
        for (uint32_t c = 0; c < n_ch; c++) {
            ChanParams &p = e->h_params[first_ch + c];
            if (e->mode_gen[first_ch + c] == mgen[c]) p.mode = mode0[c];
            if (e->rot_gen[first_ch + c] == rgen[c]) p.rotation = rot0[c];
        }
        e->params_dirty = e->lists_dirty = true;
    }
    return rc;
}

}  // extern "C"
