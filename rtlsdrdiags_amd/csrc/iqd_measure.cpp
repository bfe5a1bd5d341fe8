// Band track measurements of libiqdemod.so (include/iqdemod.h: iqd_measure_*), on the engine's stream.  Kernel: iqd_measure.hip.
#include "iqd_engine_impl.h"
#include "iqd_measure.h"

static_assert(sizeof(iqd_track_measure) == iqd::MSR_RECORD_BYTES && sizeof(iqd_measure_config) == 48, "the ABI's records");
static_assert(sizeof(iqd_track_slot) == 32 && sizeof(iqd_detect_row) == 16, "the ABI's records");

struct iqd_measure {
    iqd_t *e = nullptr;
    iqd_measure_config cfg{};
    DevBuf st_power, st_rows, st_slots, st_meas;
};

extern "C" {

int iqd_measure_create(iqd_t *e, const iqd_measure_config *cfg, iqd_measure_t **out)
{
    if (!e) return IQD_EINVAL;
    if (!out) return e->fail(IQD_EINVAL, "iqd_measure_create: out is NULL");
    if (!cfg) return e->fail(IQD_EINVAL, "iqd_measure_create: cfg is NULL");
    const uint32_t n = cfg->n_bins;
    if (cfg->n_sources == 0) return e->fail(IQD_EINVAL, "iqd_measure_create: n_sources is 0");
    if (n < MSR_MIN_BINS || n > MSR_MAX_BINS || (n & (n - 1)) != 0)
        return e->fail(IQD_EINVAL, "iqd_measure_create: n_bins (%u) must be 64, 128, 256, 512, 1024 or 2048", n);
    if (cfg->n_slots == 0 || cfg->n_slots > MSR_MAX_SLOTS) return e->fail(IQD_EINVAL, "iqd_measure_create: n_slots (%u) must be 1 .. 64", cfg->n_slots);
    if (cfg->dc_guard > n / 4) return e->fail(IQD_EINVAL, "iqd_measure_create: dc_guard (%u) must be 0 .. n_bins / 4 (%u)", cfg->dc_guard, n / 4);
    if (cfg->margin > MSR_MAX_MARGIN) return e->fail(IQD_EINVAL, "iqd_measure_create: margin (%u) must be 0 .. 64", cfg->margin);
    if (cfg->obw_tail_q16 > MSR_MAX_BETA) return e->fail(IQD_EINVAL, "iqd_measure_create: obw_tail_q16 (%u) must be 0 .. 32767", cfg->obw_tail_q16);
    if (cfg->carrier_half > MSR_MAX_CARRIER_HALF) return e->fail(IQD_EINVAL, "iqd_measure_create: carrier_half (%u) must be 0 .. 8", cfg->carrier_half);
    if (cfg->carrier_min_q8 > MSR_MAX_CARRIER_Q8)
        return e->fail(IQD_EINVAL, "iqd_measure_create: carrier_min_q8 (%u) must be 0 .. 256", cfg->carrier_min_q8);
    if (cfg->wide_bins == 0 || cfg->wide_bins > n + 1)
        return e->fail(IQD_EINVAL, "iqd_measure_create: wide_bins (%u) must be 1 .. n_bins + 1 (%u)", cfg->wide_bins, n + 1);
    for (int i = 0; i < 2; i++)
        if (cfg->reserved[i]) return e->fail(IQD_EINVAL, "iqd_measure_create: reserved[%d] is not 0", i);
    iqd_measure *m = new (std::nothrow) iqd_measure;
    if (!m) return IQD_ENOMEM;
    m->e = e;
    m->cfg = *cfg;
    *out = m;
    return IQD_OK;
}

void iqd_measure_destroy(iqd_measure_t *m)
{
    if (!m) return;
    (void)hipSetDevice(m->e->device);
    (void)hipStreamSynchronize(m->e->stream);
    delete m;
}

// the refusals of a run, before anything is queued
static int measure_run_check(iqd_measure_t *m, const void *power, const void *rows, const void *slots, size_t n_blocks, const void *meas,
                             const char *who)
{
    if (!m) return IQD_EINVAL;
    iqd_t *e = m->e;
    if (!power) return e->fail(IQD_EINVAL, "%s: power is NULL", who);
    if (!rows) return e->fail(IQD_EINVAL, "%s: rows is NULL", who);
    if (!slots) return e->fail(IQD_EINVAL, "%s: slots is NULL", who);
    if (!meas) return e->fail(IQD_EINVAL, "%s: meas is NULL", who);
    if (n_blocks == 0) return e->fail(IQD_EINVAL, "%s: n_blocks is 0", who);
    if (n_blocks > MSR_MAX_ROWS / m->cfg.n_sources)
        return e->fail(IQD_EINVAL, "%s: n_blocks (%zu) times n_sources (%u) is more than one call covers (2^31 - 1)", who, n_blocks, m->cfg.n_sources);
    return IQD_OK;
}

int iqd_measure_run_device(iqd_measure_t *m, const uint32_t *power_dev, const iqd_detect_row *rows_dev, const iqd_track_slot *slots_dev,
                           size_t n_blocks, iqd_track_measure *meas_dev)
{
    int rc = measure_run_check(m, power_dev, rows_dev, slots_dev, n_blocks, meas_dev, "iqd_measure_run_device");
    if (rc != IQD_OK) return rc;
    iqd_t *e = m->e;
    if ((uintptr_t)power_dev % 16) return e->fail(IQD_EINVAL, "iqd_measure_run_device: power_dev is not 16-byte aligned");
    if ((uintptr_t)rows_dev % 16) return e->fail(IQD_EINVAL, "iqd_measure_run_device: rows_dev is not 16-byte aligned");
    if ((uintptr_t)slots_dev % 16) return e->fail(IQD_EINVAL, "iqd_measure_run_device: slots_dev is not 16-byte aligned");
    if ((uintptr_t)meas_dev % 16) return e->fail(IQD_EINVAL, "iqd_measure_run_device: meas_dev is not 16-byte aligned");
    (void)hipSetDevice(e->device);
    const iqd_measure_config &c = m->cfg;
    MsrLaunch a{};
    a.power = power_dev; a.rows = (const uint4 *)rows_dev; a.slots = (const uint4 *)slots_dev; a.meas = (uint4 *)meas_dev;
    a.n_rows = n_blocks * c.n_sources; a.n = c.n_bins; a.n_slots = c.n_slots; a.dc_guard = c.dc_guard; a.margin = c.margin;
    a.beta = c.obw_tail_q16; a.carrier_half = c.carrier_half; a.min_sum = c.min_sum; a.carrier_min = c.carrier_min_q8;
    a.wide_bins = c.wide_bins;
    HIP_LAUNCH(e, launch_measure(a, e->stream));
    return IQD_OK;
}

int iqd_measure_run(iqd_measure_t *m, const uint32_t *power, const iqd_detect_row *rows, const iqd_track_slot *slots, size_t n_blocks,
                    iqd_track_measure *meas)
{
    int rc = measure_run_check(m, power, rows, slots, n_blocks, meas, "iqd_measure_run");
    if (rc != IQD_OK) return rc;
    iqd_t *e = m->e;
    (void)hipSetDevice(e->device);
    const size_t n_rows = n_blocks * m->cfg.n_sources;
    const size_t pb = n_rows * m->cfg.n_bins * sizeof(uint32_t), rb = n_rows * sizeof(iqd_detect_row);
    const size_t sb = n_rows * m->cfg.n_slots * sizeof(iqd_track_slot), mb = n_rows * m->cfg.n_slots * sizeof(iqd_track_measure);
    HIP_TRY(e, m->st_power.ensure(pb));
    HIP_TRY(e, m->st_rows.ensure(rb));
    HIP_TRY(e, m->st_slots.ensure(sb));
    HIP_TRY(e, m->st_meas.ensure(mb));
    HIP_COPY(e, hipMemcpyAsync(m->st_power.p, power, pb, hipMemcpyHostToDevice, e->stream));
    HIP_COPY(e, hipMemcpyAsync(m->st_rows.p, rows, rb, hipMemcpyHostToDevice, e->stream));
    HIP_COPY(e, hipMemcpyAsync(m->st_slots.p, slots, sb, hipMemcpyHostToDevice, e->stream));
    rc = iqd_measure_run_device(m, m->st_power.as<const uint32_t>(), m->st_rows.as<const iqd_detect_row>(),
                                m->st_slots.as<const iqd_track_slot>(), n_blocks, m->st_meas.as<iqd_track_measure>());
    if (rc != IQD_OK) return rc;
    HIP_COPY(e, hipMemcpyAsync(meas, m->st_meas.p, mb, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

}  // extern "C"
