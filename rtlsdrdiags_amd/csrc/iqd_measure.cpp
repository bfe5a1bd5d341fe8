// Band track measurements of libiqdemod.so (include/iqdemod.h: iqd_measure_*), on the engine's stream.  Kernel: iqd_measure.hip.
// Here: the config's ranges, the call's arrays and the launch; the skeleton around them is iqd_band_host.h.
#include "iqd_band_host.h"
#include "iqd_measure.h"

static_assert(sizeof(iqd_track_measure) == iqd::MSR_RECORD_BYTES && sizeof(iqd_measure_config) == 48, "the ABI's records");
static_assert(sizeof(iqd_track_slot) == 32 && sizeof(iqd_detect_row) == 16, "the ABI's records");
static_assert(MSR_MIN_BINS == BAND_MIN_BINS && MSR_MAX_BINS == BAND_MAX_BINS && MSR_MAX_ROWS == BAND_MAX_ROWS, "the shared refusals' bounds");

struct iqd_measure {
    iqd_t *e = nullptr;
    iqd_measure_config cfg{};
    DevBuf st_power, st_rows, st_slots, st_meas;
};

extern "C" {

int iqd_measure_create(iqd_t *e, const iqd_measure_config *cfg, iqd_measure_t **out)
{
    int rc = obj_create_check(e, cfg, out, __func__);
    if (rc != IQD_OK) return rc;
    const uint32_t n = cfg->n_bins;
    if (cfg->n_sources == 0) return e->fail(IQD_EINVAL, "iqd_measure_create: n_sources is 0");
    if ((rc = band_bins_check(e, n, __func__)) != IQD_OK) return rc;
    if (cfg->n_slots == 0 || cfg->n_slots > MSR_MAX_SLOTS) return e->fail(IQD_EINVAL, "iqd_measure_create: n_slots (%u) must be 1 .. 64", cfg->n_slots);
    if (cfg->dc_guard > n / 4) return e->fail(IQD_EINVAL, "iqd_measure_create: dc_guard (%u) must be 0 .. n_bins / 4 (%u)", cfg->dc_guard, n / 4);
    if (cfg->margin > MSR_MAX_MARGIN) return e->fail(IQD_EINVAL, "iqd_measure_create: margin (%u) must be 0 .. 64", cfg->margin);
    if (cfg->obw_tail_q16 > MSR_MAX_BETA) return e->fail(IQD_EINVAL, "iqd_measure_create: obw_tail_q16 (%u) must be 0 .. 32767", cfg->obw_tail_q16);
    if (cfg->carrier_half > MSR_MAX_CARRIER_HALF) return e->fail(IQD_EINVAL, "iqd_measure_create: carrier_half (%u) must be 0 .. 8", cfg->carrier_half);
    if (cfg->carrier_min_q8 > MSR_MAX_CARRIER_Q8)
        return e->fail(IQD_EINVAL, "iqd_measure_create: carrier_min_q8 (%u) must be 0 .. 256", cfg->carrier_min_q8);
    if (cfg->wide_bins == 0 || cfg->wide_bins > n + 1)
        return e->fail(IQD_EINVAL, "iqd_measure_create: wide_bins (%u) must be 1 .. n_bins + 1 (%u)", cfg->wide_bins, n + 1);
    if ((rc = obj_reserved_check(e, cfg->reserved, __func__)) != IQD_OK) return rc;
    iqd_measure *m = new (std::nothrow) iqd_measure;
    if (!m) return IQD_ENOMEM;
    m->e = e;
    m->cfg = *cfg;
    *out = m;
    return IQD_OK;
}

void iqd_measure_destroy(iqd_measure_t *m) { obj_destroy(m); }

// the call's arrays, as run stages them ([n_sources][n_blocks] rows throughout)
static ObjArgs<4> measure_args(iqd_measure_t *m, const void *power, const void *rows, const void *slots, size_t n_blocks, void *meas)
{
    const size_t n_rows = n_blocks * m->cfg.n_sources;
    return {{{"power", power, n_rows * m->cfg.n_bins * sizeof(uint32_t), &m->st_power, ARG_IN},
             {"rows", rows, n_rows * sizeof(iqd_detect_row), &m->st_rows, ARG_IN},
             {"slots", slots, n_rows * m->cfg.n_slots * sizeof(iqd_track_slot), &m->st_slots, ARG_IN},
             {"meas", meas, n_rows * m->cfg.n_slots * sizeof(iqd_track_measure), &m->st_meas, ARG_OUT}}};
}

int iqd_measure_run_device(iqd_measure_t *m, const uint32_t *power_dev, const iqd_detect_row *rows_dev, const iqd_track_slot *slots_dev,
                           size_t n_blocks, iqd_track_measure *meas_dev)
{
    if (!m) return IQD_EINVAL;
    iqd_t *e = m->e;
    const ObjArgs<4> args = measure_args(m, power_dev, rows_dev, slots_dev, n_blocks, meas_dev);
    int rc = band_run_check(m->e, args, n_blocks, m->cfg.n_sources, __func__);
    if (rc == IQD_OK) rc = obj_align_check(e, args, __func__);
    if (rc != IQD_OK) return rc;
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
    if (!m) return IQD_EINVAL;
    const ObjArgs<4> args = measure_args(m, power, rows, slots, n_blocks, meas);
    int rc = band_run_check(m->e, args, n_blocks, m->cfg.n_sources, __func__);
    if (rc != IQD_OK) return rc;
    return obj_staged_run(m->e, args, [&] {
        return iqd_measure_run_device(m, m->st_power.as<const uint32_t>(), m->st_rows.as<const iqd_detect_row>(),
                                      m->st_slots.as<const iqd_track_slot>(), n_blocks, m->st_meas.as<iqd_track_measure>());
    });
}

}  // extern "C"
