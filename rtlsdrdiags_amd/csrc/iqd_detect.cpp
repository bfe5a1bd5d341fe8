// The band activity detector of libiqdemod.so (include/iqdemod.h: iqd_detect_*), on the engine's stream.  Kernel: iqd_detect.hip.
// Here: the config's ranges, the call's arrays, its row count's refusals and the launch; the skeleton around them is iqd_band_host.h.
#include "iqd_band_host.h"
#include "iqd_detect.h"

static_assert(sizeof(iqd_detect_row) == iqd::DET_ROW_BYTES && sizeof(iqd_detection) == iqd::DET_RECORD_BYTES, "the ABI's records");
static_assert(DET_MIN_BINS == BAND_MIN_BINS && DET_MAX_BINS == BAND_MAX_BINS, "the shared refusals' bounds");

struct iqd_detect {
    iqd_t *e = nullptr;
    iqd_detect_config cfg{};
    DevBuf st_in, st_rows, st_det;
};

extern "C" {

int iqd_detect_offset_hz(uint32_t n_bins, uint32_t rate_hz, uint32_t centroid_q8, int64_t *hz)
{
    if (!hz || !band_bins_ok(n_bins) || rate_hz == 0 || centroid_q8 >= 256u * n_bins) return IQD_EINVAL;
    const int64_t den = 256ll * n_bins;
    const int64_t num = ((int64_t)centroid_q8 - 128ll * n_bins) * rate_hz + 128ll * n_bins;     // |num| < 2^19 x 2^32
    *hz = num / den - (num % den < 0 ? 1 : 0);
    return IQD_OK;
}

int iqd_detect_create(iqd_t *e, const iqd_detect_config *cfg, iqd_detect_t **out)
{
    int rc = obj_create_check(e, cfg, out, __func__);
    if (rc != IQD_OK) return rc;
    const uint32_t n = cfg->n_bins;
    if ((rc = band_bins_check(e, n, __func__)) != IQD_OK) return rc;
    if (cfg->floor_rank >= n) return e->fail(IQD_EINVAL, "iqd_detect_create: floor_rank (%u) must be below n_bins (%u)", cfg->floor_rank, n);
    if (cfg->ratio_q8 < DET_MIN_RATIO || cfg->ratio_q8 > DET_MAX_RATIO)
        return e->fail(IQD_EINVAL, "iqd_detect_create: ratio_q8 (%u) must be 256 .. 2^24", cfg->ratio_q8);
    if (cfg->dc_guard > n / 4) return e->fail(IQD_EINVAL, "iqd_detect_create: dc_guard (%u) must be 0 .. n_bins / 4 (%u)", cfg->dc_guard, n / 4);
    if (cfg->bridge > DET_MAX_BRIDGE) return e->fail(IQD_EINVAL, "iqd_detect_create: bridge (%u) must be 0 .. 64", cfg->bridge);
    if (cfg->min_width == 0 || cfg->min_width > n)
        return e->fail(IQD_EINVAL, "iqd_detect_create: min_width (%u) must be 1 .. n_bins (%u)", cfg->min_width, n);
    if (cfg->max_detections == 0 || cfg->max_detections > n / 2)
        return e->fail(IQD_EINVAL, "iqd_detect_create: max_detections (%u) must be 1 .. n_bins / 2 (%u)", cfg->max_detections, n / 2);
    if ((rc = obj_reserved_check(e, cfg->reserved, __func__)) != IQD_OK) return rc;
    iqd_detect *d = new (std::nothrow) iqd_detect;
    if (!d) return IQD_ENOMEM;
    d->e = e;
    d->cfg = *cfg;
    *out = d;
    return IQD_OK;
}

void iqd_detect_destroy(iqd_detect_t *d) { obj_destroy(d); }

// the call's arrays, as run stages them
static ObjArgs<3> detect_args(iqd_detect_t *d, const void *power, size_t n_rows, void *rows, void *det)
{
    return {{{"power", power, n_rows * d->cfg.n_bins * sizeof(uint32_t), &d->st_in, ARG_IN},
             {"rows", rows, n_rows * sizeof(iqd_detect_row), &d->st_rows, ARG_OUT},
             {"det", det, n_rows * d->cfg.max_detections * sizeof(iqd_detection), &d->st_det, ARG_OUT}}};
}

// rows have no sources: the count's refusals are the detector's own
static int detect_run_check(iqd_detect_t *d, const ObjArgs<3> &args, size_t n_rows, const char *who)
{
    iqd_t *e = d->e;
    int rc = obj_null_check(e, args, who);
    if (rc != IQD_OK) return rc;
    if (n_rows == 0) return e->fail(IQD_EINVAL, "%s: n_rows is 0", who);
    if (n_rows > DET_MAX_ROWS) return e->fail(IQD_EINVAL, "%s: n_rows (%zu) is more than one launch covers (2^31 - 1)", who, n_rows);
    return IQD_OK;
}

int iqd_detect_run_device(iqd_detect_t *d, const uint32_t *power_dev, size_t n_rows, iqd_detect_row *rows_dev, iqd_detection *det_dev)
{
    if (!d) return IQD_EINVAL;
    iqd_t *e = d->e;
    const ObjArgs<3> args = detect_args(d, power_dev, n_rows, rows_dev, det_dev);
    int rc = detect_run_check(d, args, n_rows, __func__);
    if (rc == IQD_OK) rc = obj_align_check(e, args, __func__);
    if (rc != IQD_OK) return rc;
    (void)hipSetDevice(e->device);
    const iqd_detect_config &c = d->cfg;
    DetLaunch a{};
    a.power = power_dev; a.rows = (uint4 *)rows_dev; a.det = (uint4 *)det_dev; a.n_rows = n_rows;
    a.n = c.n_bins; a.rank = c.floor_rank; a.ratio_q8 = c.ratio_q8; a.dc_guard = c.dc_guard; a.bridge = c.bridge;
    a.min_width = c.min_width; a.max_det = c.max_detections;
    HIP_LAUNCH(e, launch_detect(a, e->stream));
    return IQD_OK;
}

int iqd_detect_run(iqd_detect_t *d, const uint32_t *power, size_t n_rows, iqd_detect_row *rows, iqd_detection *det)
{
    if (!d) return IQD_EINVAL;
    const ObjArgs<3> args = detect_args(d, power, n_rows, rows, det);
    int rc = detect_run_check(d, args, n_rows, __func__);
    if (rc != IQD_OK) return rc;
    return obj_staged_run(d->e, args, [&] {
        return iqd_detect_run_device(d, d->st_in.as<const uint32_t>(), n_rows, d->st_rows.as<iqd_detect_row>(), d->st_det.as<iqd_detection>());
    });
}

}  // extern "C"
