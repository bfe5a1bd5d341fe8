// The band activity tracker of libiqdemod.so (include/iqdemod.h: iqd_track_*), on the engine's stream.  Kernel: iqd_track.hip.
#include "iqd_engine_impl.h"
#include "iqd_track.h"

static_assert(sizeof(iqd_track_slot) == iqd::TRK_SLOT_BYTES && sizeof(iqd_track_block) == iqd::TRK_BLOCK_BYTES, "the ABI's records");
static_assert(sizeof(iqd_detect_row) == 16 && sizeof(iqd_detection) == 32 && sizeof(iqd_track_config) == 64, "the ABI's records");

struct iqd_track {
    iqd_t *e = nullptr;
    iqd_track_config cfg{};
    DevBuf state;                        // [n_sources][S] slots, then [n_sources] next_id
    size_t slot_bytes = 0, state_bytes = 0;
    DevBuf st_rows, st_det, st_slots, st_blocks;
};

static bool track_bins_ok(uint32_t n) { return n >= TRK_MIN_BINS && n <= TRK_MAX_BINS && (n & (n - 1)) == 0; }

extern "C" {

int iqd_track_phase_inc(uint32_t n_bins, uint32_t centroid_q8, uint32_t inc_bias, uint32_t *inc)
{
    if (!inc || !track_bins_ok(n_bins) || centroid_q8 >= 256u * n_bins) return IQD_EINVAL;
    uint32_t log2n = 0;
    while ((1u << log2n) < n_bins) log2n++;
    *inc = ((centroid_q8 - 128u * n_bins) << (24 - log2n)) + inc_bias;     // mod 2^32 throughout
    return IQD_OK;
}

int iqd_track_create(iqd_t *e, const iqd_track_config *cfg, iqd_track_t **out)
{
    if (!e) return IQD_EINVAL;
    if (!out) return e->fail(IQD_EINVAL, "iqd_track_create: out is NULL");
    if (!cfg) return e->fail(IQD_EINVAL, "iqd_track_create: cfg is NULL");
    const uint32_t n = cfg->n_bins;
    if (cfg->n_sources == 0) return e->fail(IQD_EINVAL, "iqd_track_create: n_sources is 0");
    if (!track_bins_ok(n)) return e->fail(IQD_EINVAL, "iqd_track_create: n_bins (%u) must be 64, 128, 256, 512, 1024 or 2048", n);
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
    for (int i = 0; i < 4; i++)
        if (cfg->reserved[i]) return e->fail(IQD_EINVAL, "iqd_track_create: reserved[%d] is not 0", i);
    iqd_track *t = new (std::nothrow) iqd_track;
    if (!t) return IQD_ENOMEM;
    t->e = e;
    t->cfg = *cfg;
    t->slot_bytes = (size_t)cfg->n_sources * cfg->n_slots * sizeof(iqd_track_slot);
    t->state_bytes = t->slot_bytes + (size_t)cfg->n_sources * sizeof(uint32_t);
    (void)hipSetDevice(e->device);
    int rc = IQD_OK;
    if (t->state.ensure(t->state_bytes) != hipSuccess) rc = e->fail(IQD_ENOMEM, "iqd_track_create: no device memory for %zu bytes of state", t->state_bytes);
    if (rc == IQD_OK) rc = iqd_track_reset(t);
    if (rc != IQD_OK) {
        delete t;
        return rc;
    }
    *out = t;
    return IQD_OK;
}

void iqd_track_destroy(iqd_track_t *t)
{
    if (!t) return;
    (void)hipSetDevice(t->e->device);
    (void)hipStreamSynchronize(t->e->stream);
    delete t;
}

int iqd_track_reset(iqd_track_t *t)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    (void)hipSetDevice(e->device);
    HIP_COPY(e, hipMemsetAsync(t->state.p, 0, t->state_bytes, e->stream));
    return IQD_OK;
}

// the refusals of a run, before anything is queued
static int track_run_check(iqd_track_t *t, const void *rows, const void *det, size_t n_blocks, const void *slots, const void *blocks,
                           const char *who)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    if (!rows) return e->fail(IQD_EINVAL, "%s: rows is NULL", who);
    if (!det) return e->fail(IQD_EINVAL, "%s: det is NULL", who);
    if (!slots) return e->fail(IQD_EINVAL, "%s: slots is NULL", who);
    if (!blocks) return e->fail(IQD_EINVAL, "%s: blocks is NULL", who);
    if (n_blocks == 0) return e->fail(IQD_EINVAL, "%s: n_blocks is 0", who);
    if (n_blocks > TRK_MAX_ROWS / t->cfg.n_sources)
        return e->fail(IQD_EINVAL, "%s: n_blocks (%zu) times n_sources (%u) is more than one call covers (2^31 - 1)", who, n_blocks, t->cfg.n_sources);
    return IQD_OK;
}

int iqd_track_run_device(iqd_track_t *t, const iqd_detect_row *rows_dev, const iqd_detection *det_dev, size_t n_blocks,
                         iqd_track_slot *slots_dev, iqd_track_block *blocks_dev)
{
    int rc = track_run_check(t, rows_dev, det_dev, n_blocks, slots_dev, blocks_dev, "iqd_track_run_device");
    if (rc != IQD_OK) return rc;
    iqd_t *e = t->e;
    if ((uintptr_t)rows_dev % 16) return e->fail(IQD_EINVAL, "iqd_track_run_device: rows_dev is not 16-byte aligned");
    if ((uintptr_t)det_dev % 16) return e->fail(IQD_EINVAL, "iqd_track_run_device: det_dev is not 16-byte aligned");
    if ((uintptr_t)slots_dev % 16) return e->fail(IQD_EINVAL, "iqd_track_run_device: slots_dev is not 16-byte aligned");
    if ((uintptr_t)blocks_dev % 16) return e->fail(IQD_EINVAL, "iqd_track_run_device: blocks_dev is not 16-byte aligned");
    (void)hipSetDevice(e->device);
    const iqd_track_config &c = t->cfg;
    TrkLaunch a{};
    a.rows = (const uint4 *)rows_dev; a.det = (const uint4 *)det_dev; a.slots = (uint4 *)slots_dev; a.blocks = (uint4 *)blocks_dev;
    a.state = t->state.as<uint4>(); a.next_id = (uint32_t *)(t->state.as<uint8_t>() + t->slot_bytes);
    a.n_blocks = n_blocks; a.n_sources = c.n_sources; a.n = c.n_bins; a.max_det = c.max_detections; a.n_slots = c.n_slots;
    a.gate = c.gate_q8; a.open_hits = c.open_hits; a.hold = c.hold_blocks; a.alpha = c.alpha_q8; a.inc_bias = c.inc_bias;
    a.edge0 = c.class_edge[0]; a.edge1 = c.class_edge[1]; a.edge2 = c.class_edge[2];
    HIP_LAUNCH(e, launch_track(a, e->stream));
    return IQD_OK;
}

int iqd_track_run(iqd_track_t *t, const iqd_detect_row *rows, const iqd_detection *det, size_t n_blocks, iqd_track_slot *slots,
                  iqd_track_block *blocks)
{
    int rc = track_run_check(t, rows, det, n_blocks, slots, blocks, "iqd_track_run");
    if (rc != IQD_OK) return rc;
    iqd_t *e = t->e;
    (void)hipSetDevice(e->device);
    const size_t n_rows = n_blocks * t->cfg.n_sources;
    const size_t rb = n_rows * sizeof(iqd_detect_row), db = n_rows * t->cfg.max_detections * sizeof(iqd_detection);
    const size_t sb = n_rows * t->cfg.n_slots * sizeof(iqd_track_slot), bb = n_rows * sizeof(iqd_track_block);
    HIP_TRY(e, t->st_rows.ensure(rb));
    HIP_TRY(e, t->st_det.ensure(db));
    HIP_TRY(e, t->st_slots.ensure(sb));
    HIP_TRY(e, t->st_blocks.ensure(bb));
    HIP_COPY(e, hipMemcpyAsync(t->st_rows.p, rows, rb, hipMemcpyHostToDevice, e->stream));
    HIP_COPY(e, hipMemcpyAsync(t->st_det.p, det, db, hipMemcpyHostToDevice, e->stream));
    rc = iqd_track_run_device(t, t->st_rows.as<const iqd_detect_row>(), t->st_det.as<const iqd_detection>(), n_blocks,
                              t->st_slots.as<iqd_track_slot>(), t->st_blocks.as<iqd_track_block>());
    if (rc != IQD_OK) return rc;
    HIP_COPY(e, hipMemcpyAsync(slots, t->st_slots.p, sb, hipMemcpyDeviceToHost, e->stream));
    HIP_COPY(e, hipMemcpyAsync(blocks, t->st_blocks.p, bb, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

int iqd_track_get_state(iqd_track_t *t, uint32_t source, iqd_track_slot *out)
{
    if (!t) return IQD_EINVAL;
    iqd_t *e = t->e;
    if (!out) return e->fail(IQD_EINVAL, "iqd_track_get_state: out is NULL");
    if (source >= t->cfg.n_sources) return e->fail(IQD_EINVAL, "iqd_track_get_state: source (%u) must be below n_sources (%u)", source, t->cfg.n_sources);
    (void)hipSetDevice(e->device);
    const size_t bytes = (size_t)t->cfg.n_slots * sizeof(iqd_track_slot);
    HIP_COPY(e, hipMemcpyAsync(out, t->state.as<uint8_t>() + source * bytes, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

}  // extern "C"
