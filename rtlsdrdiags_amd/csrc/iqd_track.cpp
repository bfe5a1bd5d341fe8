// The band activity tracker of libiqdemod.so (include/iqdemod.h: iqd_track_*), on the engine's stream.  Kernel: iqd_track.hip.
// Here: the config's ranges, the call's arrays and the launch; the skeleton around them is iqd_band_host.h.
#include "iqd_band_host.h"
#include "iqd_track.h"

static_assert(sizeof(iqd_track_slot) == iqd::TRK_SLOT_BYTES && sizeof(iqd_track_block) == iqd::TRK_BLOCK_BYTES, "the ABI's records");
static_assert(sizeof(iqd_detect_row) == 16 && sizeof(iqd_detection) == 32 && sizeof(iqd_track_config) == 64, "the ABI's records");
static_assert(TRK_MIN_BINS == BAND_MIN_BINS && TRK_MAX_BINS == BAND_MAX_BINS && TRK_MAX_ROWS == BAND_MAX_ROWS, "the shared refusals' bounds");

struct iqd_track {
    iqd_t *e = nullptr;
    iqd_track_config cfg{};
    BandState state;                     // [n_sources][S] slots, then [n_sources] next_id
    DevBuf st_rows, st_det, st_slots, st_blocks;
};

extern "C" {

int iqd_track_phase_inc(uint32_t n_bins, uint32_t centroid_q8, uint32_t inc_bias, uint32_t *inc)
{
    if (!inc || !band_bins_ok(n_bins) || centroid_q8 >= 256u * n_bins) return IQD_EINVAL;
    uint32_t log2n = 0;
    while ((1u << log2n) < n_bins) log2n++;
    *inc = ((centroid_q8 - 128u * n_bins) << (24 - log2n)) + inc_bias;     // mod 2^32 throughout
    return IQD_OK;
}

int iqd_track_create(iqd_t *e, const iqd_track_config *cfg, iqd_track_t **out)
{
    int rc = obj_create_check(e, cfg, out, __func__);
    if (rc != IQD_OK) return rc;
    const uint32_t n = cfg->n_bins;
    if (cfg->n_sources == 0) return e->fail(IQD_EINVAL, "iqd_track_create: n_sources is 0");
    if ((rc = band_bins_check(e, n, __func__)) != IQD_OK) return rc;
    if (cfg->max_detections == 0 || cfg->max_detections > n / 2)
        return e->fail(IQD_EINVAL, "iqd_track_create: max_detections (%u) must be 1 .. n_bins / 2 (%u)", cfg->max_detections, n / 2);
    if (cfg->n_slots == 0 || cfg->n_slots > TRK_MAX_SLOTS) return e->fail(IQD_EINVAL, "iqd_track_create: n_slots (%u) must be 1 .. 64", cfg->n_slots);
    if (cfg->gate_q8 >= 256u * n) return e->fail(IQD_EINVAL, "iqd_track_create: gate_q8 (%u) must be 0 .. 256 n_bins - 1 (%u)", cfg->gate_q8, 256u * n - 1);
    if (cfg->open_hits == 0 || cfg->open_hits > TRK_MAX_OPEN) return e->fail(IQD_EINVAL, "iqd_track_create: open_hits (%u) must be 1 .. 255", cfg->open_hits);
    if (cfg->hold_blocks > TRK_MAX_HOLD) return e->fail(IQD_EINVAL, "iqd_track_create: hold_blocks (%u) must be 0 .. 65535", cfg->hold_blocks);
    if (cfg->alpha_q8 == 0 || cfg->alpha_q8 > TRK_MAX_ALPHA) return e->fail(IQD_EINVAL, "iqd_track_create: alpha_q8 (%u) must be 1 .. 256", cfg->alpha_q8);
    const uint32_t *ce = cfg->class_edge;
    if (ce[0] < 1 || ce[0] > ce[1] || ce[1] > ce[2] || ce[2] > n + 1)
        return e->fail(IQD_EINVAL, "iqd_track_create: class_edge (%u, %u, %u) must be 1 <= e0 <= e1 <= e2 <= n_bins + 1 (%u)", ce[0], ce[1], ce[2], n + 1);
    if ((rc = obj_reserved_check(e, cfg->reserved, __func__)) != IQD_OK) return rc;
    iqd_track *t = new (std::nothrow) iqd_track;
    if (!t) return IQD_ENOMEM;
    t->e = e;
    t->cfg = *cfg;
    if ((rc = t->state.create(e, cfg->n_sources, cfg->n_slots * sizeof(iqd_track_slot), sizeof(uint32_t), __func__)) == IQD_OK) *out = t;
    else delete t;
    return rc;
}

void iqd_track_destroy(iqd_track_t *t) { obj_destroy(t); }

int iqd_track_reset(iqd_track_t *t) { return t ? t->state.reset(t->e) : IQD_EINVAL; }

// the call's arrays, as run stages them ([n_sources][n_blocks] rows throughout)
static ObjArgs<4> track_args(iqd_track_t *t, const void *rows, const void *det, size_t n_blocks, void *slots, void *blocks)
{
    const size_t n_rows = n_blocks * t->cfg.n_sources;
    return {{{"rows", rows, n_rows * sizeof(iqd_detect_row), &t->st_rows, ARG_IN},
             {"det", det, n_rows * t->cfg.max_detections * sizeof(iqd_detection), &t->st_det, ARG_IN},
             {"slots", slots, n_rows * t->cfg.n_slots * sizeof(iqd_track_slot), &t->st_slots, ARG_OUT},
             {"blocks", blocks, n_rows * sizeof(iqd_track_block), &t->st_blocks, ARG_OUT}}};
}

int iqd_track_run_device(iqd_track_t *t, const iqd_detect_row *rows_dev, const iqd_detection *det_dev, size_t n_blocks,
                         iqd_track_slot *slots_dev, iqd_track_block *blocks_dev)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    const ObjArgs<4> args = track_args(t, rows_dev, det_dev, n_blocks, slots_dev, blocks_dev);
    int rc = band_run_check(t->e, args, n_blocks, t->cfg.n_sources, __func__);
    if (rc == IQD_OK) rc = obj_align_check(e, args, __func__);
    if (rc != IQD_OK) return rc;
    (void)hipSetDevice(e->device);
    const iqd_track_config &c = t->cfg;
    TrkLaunch a{};
    a.rows = (const uint4 *)rows_dev; a.det = (const uint4 *)det_dev; a.slots = (uint4 *)slots_dev; a.blocks = (uint4 *)blocks_dev;
    a.state = t->state.buf.as<uint4>(); a.next_id = (uint32_t *)t->state.tails();
    a.n_blocks = n_blocks; a.n_sources = c.n_sources; a.n = c.n_bins; a.max_det = c.max_detections; a.n_slots = c.n_slots;
    a.gate = c.gate_q8; a.open_hits = c.open_hits; a.hold = c.hold_blocks; a.alpha = c.alpha_q8; a.inc_bias = c.inc_bias;
    a.edge0 = c.class_edge[0]; a.edge1 = c.class_edge[1]; a.edge2 = c.class_edge[2];
    HIP_LAUNCH(e, launch_track(a, e->stream));
    return IQD_OK;
}

int iqd_track_run(iqd_track_t *t, const iqd_detect_row *rows, const iqd_detection *det, size_t n_blocks, iqd_track_slot *slots,
                  iqd_track_block *blocks)
{
    if (!t) return IQD_EINVAL;
    const ObjArgs<4> args = track_args(t, rows, det, n_blocks, slots, blocks);
    int rc = band_run_check(t->e, args, n_blocks, t->cfg.n_sources, __func__);
    if (rc != IQD_OK) return rc;
    return obj_staged_run(t->e, args, [&] {
        return iqd_track_run_device(t, t->st_rows.as<const iqd_detect_row>(), t->st_det.as<const iqd_detection>(), n_blocks,
                                    t->st_slots.as<iqd_track_slot>(), t->st_blocks.as<iqd_track_block>());
    });
}

int iqd_track_get_state(iqd_track_t *t, uint32_t source, iqd_track_slot *out)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    if (!out) return e->fail(IQD_EINVAL, "iqd_track_get_state: out is NULL");
    return t->state.read(e, source, out, nullptr, __func__);
}

}  // extern "C"
