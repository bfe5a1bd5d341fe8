// The band track log of libiqdemod.so (include/iqdemod.h: iqd_tracklog_*), on the engine's stream.  Kernel: iqd_tracklog.hip.
#include "iqd_engine_impl.h"
#include "iqd_tracklog.h"

static_assert(sizeof(iqd_track_summary) == iqd::TLG_SUMMARY_BYTES && sizeof(iqd_tracklog_counts) == iqd::TLG_COUNTS_BYTES, "the ABI's records");
static_assert(sizeof(iqd_tracklog_config) == 32 && sizeof(iqd_track_slot) == 32 && sizeof(iqd_track_measure) == 32, "the ABI's records");

struct iqd_tracklog {
    iqd_t *e = nullptr;
    iqd_tracklog_config cfg{};
    DevBuf state;                        // [n_sources][S] summaries, then [n_sources] block indices
    size_t summary_bytes = 0, state_bytes = 0;
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
    if (!e) return IQD_EINVAL;
    if (!out) return e->fail(IQD_EINVAL, "iqd_tracklog_create: out is NULL");
    if (!cfg) return e->fail(IQD_EINVAL, "iqd_tracklog_create: cfg is NULL");
    if (cfg->n_sources == 0) return e->fail(IQD_EINVAL, "iqd_tracklog_create: n_sources is 0");
    if (cfg->n_slots == 0 || cfg->n_slots > TLG_MAX_SLOTS) return e->fail(IQD_EINVAL, "iqd_tracklog_create: n_slots (%u) must be 1 .. 64", cfg->n_slots);
    if (cfg->max_events == 0 || cfg->max_events > TLG_MAX_EVENTS)
        return e->fail(IQD_EINVAL, "iqd_tracklog_create: max_events (%u) must be 1 .. 65536", cfg->max_events);
    if (cfg->min_active == 0 || cfg->min_active > TLG_MAX_MIN_ACTIVE)
        return e->fail(IQD_EINVAL, "iqd_tracklog_create: min_active (%u) must be 1 .. 65535", cfg->min_active);
    if (cfg->vote_min == 0 || cfg->vote_min > TLG_MAX_VOTE_MIN)
        return e->fail(IQD_EINVAL, "iqd_tracklog_create: vote_min (%u) must be 1 .. 65535", cfg->vote_min);
    for (int i = 0; i < 3; i++)
        if (cfg->reserved[i]) return e->fail(IQD_EINVAL, "iqd_tracklog_create: reserved[%d] is not 0", i);
    iqd_tracklog *t = new (std::nothrow) iqd_tracklog;
    if (!t) return IQD_ENOMEM;
    t->e = e;
    t->cfg = *cfg;
    t->summary_bytes = (size_t)cfg->n_sources * cfg->n_slots * sizeof(iqd_track_summary);
    t->state_bytes = t->summary_bytes + (size_t)cfg->n_sources * sizeof(uint64_t);
    (void)hipSetDevice(e->device);
    int rc = IQD_OK;
    if (t->state.ensure(t->state_bytes) != hipSuccess) rc = e->fail(IQD_ENOMEM, "iqd_tracklog_create: no device memory for %zu bytes of state", t->state_bytes);
    if (rc == IQD_OK) rc = iqd_tracklog_reset(t);
    if (rc != IQD_OK) {
        delete t;
        return rc;
    }
    *out = t;
    return IQD_OK;
}

void iqd_tracklog_destroy(iqd_tracklog_t *t)
{
    if (!t) return;
    (void)hipSetDevice(t->e->device);
    (void)hipStreamSynchronize(t->e->stream);
    delete t;
}

int iqd_tracklog_reset(iqd_tracklog_t *t)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    (void)hipSetDevice(e->device);
    HIP_COPY(e, hipMemsetAsync(t->state.p, 0, t->state_bytes, e->stream));
    return IQD_OK;
}

// the refusals of a run, before anything is queued
static int tracklog_run_check(iqd_tracklog_t *t, const void *slots, const void *meas, size_t n_blocks, const void *summary, const void *events,
                              const void *counts, const char *who)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    if (!slots) return e->fail(IQD_EINVAL, "%s: slots is NULL", who);
    if (!meas) return e->fail(IQD_EINVAL, "%s: meas is NULL", who);
    if (!summary) return e->fail(IQD_EINVAL, "%s: summary is NULL", who);
    if (!events) return e->fail(IQD_EINVAL, "%s: events is NULL", who);
    if (!counts) return e->fail(IQD_EINVAL, "%s: counts is NULL", who);
    if (n_blocks == 0) return e->fail(IQD_EINVAL, "%s: n_blocks is 0", who);
    if (n_blocks > TLG_MAX_ROWS / t->cfg.n_sources)
        return e->fail(IQD_EINVAL, "%s: n_blocks (%zu) times n_sources (%u) is more than one call covers (2^31 - 1)", who, n_blocks, t->cfg.n_sources);
    return IQD_OK;
}

int iqd_tracklog_run_device(iqd_tracklog_t *t, const iqd_track_slot *slots_dev, const iqd_track_measure *meas_dev, size_t n_blocks,
                            iqd_track_summary *summary_dev, iqd_track_summary *events_dev, iqd_tracklog_counts *counts_dev)
{
    int rc = tracklog_run_check(t, slots_dev, meas_dev, n_blocks, summary_dev, events_dev, counts_dev, "iqd_tracklog_run_device");
    if (rc != IQD_OK) return rc;
    iqd_t *e = t->e;
    if ((uintptr_t)slots_dev % 16) return e->fail(IQD_EINVAL, "iqd_tracklog_run_device: slots_dev is not 16-byte aligned");
    if ((uintptr_t)meas_dev % 16) return e->fail(IQD_EINVAL, "iqd_tracklog_run_device: meas_dev is not 16-byte aligned");
    if ((uintptr_t)summary_dev % 16) return e->fail(IQD_EINVAL, "iqd_tracklog_run_device: summary_dev is not 16-byte aligned");
    if ((uintptr_t)events_dev % 16) return e->fail(IQD_EINVAL, "iqd_tracklog_run_device: events_dev is not 16-byte aligned");
    if ((uintptr_t)counts_dev % 16) return e->fail(IQD_EINVAL, "iqd_tracklog_run_device: counts_dev is not 16-byte aligned");
    (void)hipSetDevice(e->device);
    const iqd_tracklog_config &c = t->cfg;
    TlgLaunch a{};
    a.slots = (const uint4 *)slots_dev; a.meas = (const uint4 *)meas_dev; a.summary = (uint4 *)summary_dev; a.events = (uint4 *)events_dev;
    a.counts = (uint4 *)counts_dev; a.state = t->state.as<uint4>(); a.g = (uint64_t *)(t->state.as<uint8_t>() + t->summary_bytes);
    a.n_blocks = n_blocks; a.n_sources = c.n_sources; a.n_slots = c.n_slots; a.max_events = c.max_events; a.min_active = c.min_active;
    a.vote_min = c.vote_min;
    HIP_LAUNCH(e, launch_tracklog(a, e->stream));
    return IQD_OK;
}

int iqd_tracklog_run(iqd_tracklog_t *t, const iqd_track_slot *slots, const iqd_track_measure *meas, size_t n_blocks, iqd_track_summary *summary,
                     iqd_track_summary *events, iqd_tracklog_counts *counts)
{
    int rc = tracklog_run_check(t, slots, meas, n_blocks, summary, events, counts, "iqd_tracklog_run");
    if (rc != IQD_OK) return rc;
    iqd_t *e = t->e;
    (void)hipSetDevice(e->device);
    const iqd_tracklog_config &c = t->cfg;
    const size_t n_entries = n_blocks * c.n_sources * c.n_slots;
    const size_t sb = n_entries * sizeof(iqd_track_slot), mb = n_entries * sizeof(iqd_track_measure), ub = n_entries * sizeof(iqd_track_summary);
    const size_t eb = (size_t)c.n_sources * c.max_events * sizeof(iqd_track_summary), cb = (size_t)c.n_sources * sizeof(iqd_tracklog_counts);
    HIP_TRY(e, t->st_slots.ensure(sb));
    HIP_TRY(e, t->st_meas.ensure(mb));
    HIP_TRY(e, t->st_summary.ensure(ub));
    HIP_TRY(e, t->st_events.ensure(eb));
    HIP_TRY(e, t->st_counts.ensure(cb));
    HIP_COPY(e, hipMemcpyAsync(t->st_slots.p, slots, sb, hipMemcpyHostToDevice, e->stream));
    HIP_COPY(e, hipMemcpyAsync(t->st_meas.p, meas, mb, hipMemcpyHostToDevice, e->stream));
    rc = iqd_tracklog_run_device(t, t->st_slots.as<const iqd_track_slot>(), t->st_meas.as<const iqd_track_measure>(), n_blocks,
                                 t->st_summary.as<iqd_track_summary>(), t->st_events.as<iqd_track_summary>(),
                                 t->st_counts.as<iqd_tracklog_counts>());
    if (rc != IQD_OK) return rc;
    HIP_COPY(e, hipMemcpyAsync(summary, t->st_summary.p, ub, hipMemcpyDeviceToHost, e->stream));
    HIP_COPY(e, hipMemcpyAsync(events, t->st_events.p, eb, hipMemcpyDeviceToHost, e->stream));
    HIP_COPY(e, hipMemcpyAsync(counts, t->st_counts.p, cb, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

int iqd_tracklog_get_state(iqd_tracklog_t *t, uint32_t source, iqd_track_summary *out, uint64_t *next_block)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    if (!out) return e->fail(IQD_EINVAL, "iqd_tracklog_get_state: out is NULL");
    if (!next_block) return e->fail(IQD_EINVAL, "iqd_tracklog_get_state: next_block is NULL");
    if (source >= t->cfg.n_sources)
        return e->fail(IQD_EINVAL, "iqd_tracklog_get_state: source (%u) must be below n_sources (%u)", source, t->cfg.n_sources);
    (void)hipSetDevice(e->device);
    const size_t bytes = (size_t)t->cfg.n_slots * sizeof(iqd_track_summary);
    HIP_COPY(e, hipMemcpyAsync(out, t->state.as<uint8_t>() + source * bytes, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_COPY(e, hipMemcpyAsync(next_block, t->state.as<uint8_t>() + t->summary_bytes + source * sizeof(uint64_t), sizeof(uint64_t),
                               hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

}  // extern "C"
