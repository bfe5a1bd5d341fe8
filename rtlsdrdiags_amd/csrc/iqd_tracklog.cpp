// The band track log of libiqdemod.so (include/iqdemod.h: iqd_tracklog_*), on the engine's stream.  Kernel: iqd_tracklog.hip.
// Here: the config's ranges, the call's arrays and the launch; the skeleton around them is iqd_band_host.h.
#include "iqd_band_host.h"
#include "iqd_tracklog.h"

static_assert(sizeof(iqd_track_summary) == iqd::TLG_SUMMARY_BYTES && sizeof(iqd_tracklog_counts) == iqd::TLG_COUNTS_BYTES, "the ABI's records");
static_assert(sizeof(iqd_tracklog_config) == 32 && sizeof(iqd_track_slot) == 32 && sizeof(iqd_track_measure) == 32, "the ABI's records");
static_assert(TLG_MAX_ROWS == BAND_MAX_ROWS, "the shared refusals' bounds");

struct iqd_tracklog {
    iqd_t *e = nullptr;
    iqd_tracklog_config cfg{};
    BandState state;                     // [n_sources][S] summaries, then [n_sources] block indices
    DevBuf st_slots, st_meas, st_summary, st_events, st_counts;
};

extern "C" {

int iqd_tracklog_mean_centre(uint64_t sum_centre_q8, uint32_t n_active, uint32_t *centre_q8)
{
    if (!centre_q8 || n_active == 0 || sum_centre_q8 / n_active > 0xffffffffull) return IQD_EINVAL;
    *centre_q8 = (uint32_t)(sum_centre_q8 / n_active);
    return IQD_OK;
}

int iqd_tracklog_create(iqd_t *e, const iqd_tracklog_config *cfg, iqd_tracklog_t **out)
{
    int rc = obj_create_check(e, cfg, out, __func__);
    if (rc != IQD_OK) return rc;
    if (cfg->n_sources == 0) return e->fail(IQD_EINVAL, "iqd_tracklog_create: n_sources is 0");
    if (cfg->n_slots == 0 || cfg->n_slots > TLG_MAX_SLOTS) return e->fail(IQD_EINVAL, "iqd_tracklog_create: n_slots (%u) must be 1 .. 64", cfg->n_slots);
    if (cfg->max_events == 0 || cfg->max_events > TLG_MAX_EVENTS)
        return e->fail(IQD_EINVAL, "iqd_tracklog_create: max_events (%u) must be 1 .. 65536", cfg->max_events);
    if (cfg->min_active == 0 || cfg->min_active > TLG_MAX_MIN_ACTIVE)
        return e->fail(IQD_EINVAL, "iqd_tracklog_create: min_active (%u) must be 1 .. 65535", cfg->min_active);
    if (cfg->vote_min == 0 || cfg->vote_min > TLG_MAX_VOTE_MIN)
        return e->fail(IQD_EINVAL, "iqd_tracklog_create: vote_min (%u) must be 1 .. 65535", cfg->vote_min);
    if ((rc = obj_reserved_check(e, cfg->reserved, __func__)) != IQD_OK) return rc;
    iqd_tracklog *t = new (std::nothrow) iqd_tracklog;
    if (!t) return IQD_ENOMEM;
    t->e = e;
    t->cfg = *cfg;
    if ((rc = t->state.create(e, cfg->n_sources, cfg->n_slots * sizeof(iqd_track_summary), sizeof(uint64_t), __func__)) == IQD_OK) *out = t;
    else delete t;
    return rc;
}

void iqd_tracklog_destroy(iqd_tracklog_t *t) { obj_destroy(t); }

int iqd_tracklog_reset(iqd_tracklog_t *t) { return t ? t->state.reset(t->e) : IQD_EINVAL; }

// the call's arrays, as run stages them: [n_sources][n_blocks][S] entries in and out, the events and counts per source
static ObjArgs<5> tracklog_args(iqd_tracklog_t *t, const void *slots, const void *meas, size_t n_blocks, void *summary, void *events, void *counts)
{
    const iqd_tracklog_config &c = t->cfg;
    const size_t n_entries = n_blocks * c.n_sources * c.n_slots;
    return {{{"slots", slots, n_entries * sizeof(iqd_track_slot), &t->st_slots, ARG_IN},
             {"meas", meas, n_entries * sizeof(iqd_track_measure), &t->st_meas, ARG_IN},
             {"summary", summary, n_entries * sizeof(iqd_track_summary), &t->st_summary, ARG_OUT},
             {"events", events, (size_t)c.n_sources * c.max_events * sizeof(iqd_track_summary), &t->st_events, ARG_OUT},
             {"counts", counts, (size_t)c.n_sources * sizeof(iqd_tracklog_counts), &t->st_counts, ARG_OUT}}};
}

int iqd_tracklog_run_device(iqd_tracklog_t *t, const iqd_track_slot *slots_dev, const iqd_track_measure *meas_dev, size_t n_blocks,
                            iqd_track_summary *summary_dev, iqd_track_summary *events_dev, iqd_tracklog_counts *counts_dev)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    const ObjArgs<5> args = tracklog_args(t, slots_dev, meas_dev, n_blocks, summary_dev, events_dev, counts_dev);
    int rc = band_run_check(t->e, args, n_blocks, t->cfg.n_sources, __func__);
    if (rc == IQD_OK) rc = obj_align_check(e, args, __func__);
    if (rc != IQD_OK) return rc;
    (void)hipSetDevice(e->device);
    const iqd_tracklog_config &c = t->cfg;
    TlgLaunch a{};
    a.slots = (const uint4 *)slots_dev; a.meas = (const uint4 *)meas_dev; a.summary = (uint4 *)summary_dev; a.events = (uint4 *)events_dev;
    a.counts = (uint4 *)counts_dev; a.state = t->state.buf.as<uint4>(); a.g = (uint64_t *)t->state.tails();
    a.n_blocks = n_blocks; a.n_sources = c.n_sources; a.n_slots = c.n_slots; a.max_events = c.max_events; a.min_active = c.min_active;
    a.vote_min = c.vote_min;
    HIP_LAUNCH(e, launch_tracklog(a, e->stream));
    return IQD_OK;
}

int iqd_tracklog_run(iqd_tracklog_t *t, const iqd_track_slot *slots, const iqd_track_measure *meas, size_t n_blocks, iqd_track_summary *summary,
                     iqd_track_summary *events, iqd_tracklog_counts *counts)
{
    if (!t) return IQD_EINVAL;
    const ObjArgs<5> args = tracklog_args(t, slots, meas, n_blocks, summary, events, counts);
    int rc = band_run_check(t->e, args, n_blocks, t->cfg.n_sources, __func__);
    if (rc != IQD_OK) return rc;
    return obj_staged_run(t->e, args, [&] {
        return iqd_tracklog_run_device(t, t->st_slots.as<const iqd_track_slot>(), t->st_meas.as<const iqd_track_measure>(), n_blocks,
                                       t->st_summary.as<iqd_track_summary>(), t->st_events.as<iqd_track_summary>(),
                                       t->st_counts.as<iqd_tracklog_counts>());
    });
}

int iqd_tracklog_get_state(iqd_tracklog_t *t, uint32_t source, iqd_track_summary *out, uint64_t *next_block)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    if (!out) return e->fail(IQD_EINVAL, "iqd_tracklog_get_state: out is NULL");
    if (!next_block) return e->fail(IQD_EINVAL, "iqd_tracklog_get_state: next_block is NULL");
    return t->state.read(e, source, out, next_block, __func__);
}

}  // extern "C"
