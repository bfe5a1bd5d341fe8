// libiqdemod.so — C-ABI (include/iqdemod.h) over the gfx950 kernels.
//
// Host orchestration only: parameter mirrors, per-call bucketing of channels by demodulator
// family, launch planning, the exact-state verification of the WBFM tile hand-offs and the
// copies of the host-pointer entry point.  There is no CPU data path in this library: every
// sample is demodulated by the HIP kernels in iqd_kernels.hip, and creation fails when no HIP
// device is usable.
// This file: the engine's lifecycle, its setters and getters, AGC and scanner, traces and stats.  The accept path is
// iqd_accept.cpp, the resamplers iqd_resampler.cpp, the memory utilities and the front end alone iqd_devmem.cpp.
#include "iqd_engine_impl.h"
#include "iqd_chan.h"

// The channelizer (iqd_chan.cpp, iqd_chan_survey.cpp) reports through the engine's error text and needs its call geometry.
namespace iqd {
int engine_fail(iqd_t *e, int code, const char *msg) { return e->fail(code, "%s", msg); }
void engine_geometry(const iqd_t *e, uint32_t *n_ch, uint32_t *block_bytes, uint32_t *flags)
{
    *n_ch = e->n_ch;
    *block_bytes = e->block_bytes;
    *flags = e->flags;
}

int engine_settle(iqd_t *e, ChzScanLaunch *s)
{
    {
        std::lock_guard<std::mutex> lk(e->mu);
        int rc = upload_params(e);
        if (rc == IQD_OK) rc = agc_sync(e);
        if (rc != IQD_OK) return rc;
    }
    s->params = e->d_params;
    s->agc_cfg = e->d_agc_cfg;
    s->agc = e->d_agc;
    s->scan_cfg = e->d_scan_cfg;
    s->scan = e->d_scan;
    s->tracker = e->d_tracker;
    HIP_TRY(e, consts_address(&s->consts));
    return IQD_OK;
}
}  // namespace iqd

// iqd_config::flags and the measurement knobs of the environment, read once per engine at its creation (include/iqdemod.h)
static void fill_knobs(PlanKnobs &kn, uint32_t flags, uint32_t n_cus)
{
    kn.flags = flags;
    kn.n_cus = n_cus;
    kn.wbfm_chunk = WBFM_CHUNK; kn.wbfm_cold_halo = COLD_HALO; kn.ch_chunk = CH_CHUNK; kn.dc_tile = DC_TILE;
    if (const char *env = getenv("IQD_WBFM_PATH")) kn.env_path = env[0] == 's' ? 1 : env[0] == 't' ? -1 : 0;
    kn.env_full_grid = getenv("IQD_FULL_GRID") != nullptr;
    if (const char *env = getenv("IQD_SHARES")) kn.env_shares_by_cost = env[0] == 'c';
    if (const char *env = getenv("IQD_FAMILY_NS")) {
        float w[FAM_COUNT];
        if (sscanf(env, "%f,%f,%f,%f", &w[0], &w[1], &w[2], &w[3]) == 4 && w[0] > 0.f && w[1] > 0.f && w[2] > 0.f && w[3] > 0.f)
            for (int f = 0; f < FAM_COUNT; f++) kn.fam_ns[f] = w[f];
    }
    if (const char *env = getenv("IQD_D4_GRAN")) kn.env_d4_gran = (uint32_t)atoi(env);
    if (const char *env = getenv("IQD_D4_LEADFREE")) kn.d4_leadfree = atoi(env);
    if (const char *env = getenv("IQD_STREAM_MIN_SEG")) kn.env_stream_min_seg = atoi(env) > 0 ? (uint64_t)atoi(env) : 0;
    if (const char *env = getenv("IQD_AM_STREAM_MIN")) kn.env_am_stream_min = atoi(env) > 0 ? (uint32_t)atoi(env) : AM_STREAM_MIN_PCM;
    if (const char *env = getenv("IQD_MIXED")) kn.env_mixed_forked = env[0] == 'f' && env[1] == 'o';
    if (const char *env = getenv("IQD_FAMILY_WEIGHTS")) {   // "am,fm,wbfm,ssb" (measurement runs)
        float w[FAM_COUNT];
        if (sscanf(env, "%f,%f,%f,%f", &w[0], &w[1], &w[2], &w[3]) == 4 && w[0] > 0 && w[1] > 0 && w[2] > 0 && w[3] > 0)
            for (int f = 0; f < FAM_COUNT; f++) kn.fam_weight[f] = w[f];
    }
    if (const char *env = getenv("IQD_STREAM_WGS")) kn.env_stream_wgs = atoi(env) > 0 ? (uint32_t)atoi(env) : 0u;
    if (const char *env = getenv("IQD_STREAM_GRAN")) kn.env_stream_gran = (uint32_t)atoi(env);
    if (const char *env = getenv("IQD_PLAN_CHUNKS")) kn.env_plan_chunks = atoi(env) > 0 ? (uint32_t)atoi(env) : 0u;
    if (const char *env = getenv("IQD_RINGS")) kn.env_rings = atoi(env) > 0 ? (uint32_t)atoi(env) : 0u;
}

extern "C" {

uint32_t iqd_abi_version(void) { return IQD_ABI_VERSION; }

const char *iqd_strerror(int status)
{
    switch (status) {
    case IQD_OK: return "ok";
    case IQD_EALREADY: return "already in the requested state";
    case IQD_EINVAL: return "invalid argument";
    case IQD_ENODEV: return "no usable HIP device";
    case IQD_ENOMEM: return "out of memory";
    case IQD_EHIP: return "HIP runtime error";
    case IQD_ESTATE: return "exact-state verification failed";
    default: return "unknown status";
    }
}

const char *iqd_last_error(iqd_t *e) { return e ? e->last_error.c_str() : "null engine"; }

int iqd_create(const iqd_config *cfg, iqd_t **out)
{
    if (!cfg || !out || cfg->abi_version != IQD_ABI_VERSION || cfg->n_channels == 0) return IQD_EINVAL;
    uint32_t bb = cfg->block_bytes ? cfg->block_bytes : 32768u;
    if (bb % 256u != 0 || bb > 32768u) return IQD_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return IQD_ENODEV;
    int dev = cfg->device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) return IQD_ENODEV;
    }
    if (dev >= ndev || hipSetDevice(dev) != hipSuccess) return IQD_ENODEV;

    iqd_t *e = new (std::nothrow) iqd_engine;
    if (!e) return IQD_ENOMEM;
    e->device = dev;
    {
        hipDeviceProp_t prop;
        e->n_cus = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
    }
    e->n_ch = cfg->n_channels;
    e->block_bytes = bb;
    e->block_samples = bb / 2;
    e->flags = cfg->flags;
    fill_knobs(e->knobs, cfg->flags, e->n_cus);
    build_consts(e->consts);
    e->h_params.resize(e->n_ch);
    for (auto &p : e->h_params) default_params(p);
    // AutomaticGainControl constructor defaults (AutomaticGainControl.cc:113-189; operating point: Radio.cc:184)
    AgcConfig agc0{};
    agc0.enabled = 0; agc0.type = 1; agc0.operating_point = -12; agc0.deadband = 1; agc0.alpha = 0.8f;
    agc0.blanking_limit = 1; agc0.reset_blanking = 0; agc0.set_gain = 0xffffffffu;
    e->h_agc.assign(e->n_ch, agc0);
    e->agc_touched.assign(e->n_ch, 0);
    AgcState st0{};
    st0.rx_gain = 24; st0.if_gain = 24; st0.filtered = 24.f; st0.normalized = -24; st0.signal_magnitude = 64;
    std::vector<AgcState> agc_states(e->n_ch, st0);
    e->k_applied.resize(2 * (size_t)e->n_ch);
    e->wbfm_epoch_left.assign(e->n_ch, 0u);
    e->wbfm_epoch_seq.assign(e->n_ch, 0u);
    for (uint32_t c = 0; c < e->n_ch; c++) {
        e->k_applied[2 * c] = e->h_params[c].wbfm_k;
        e->k_applied[2 * c + 1] = e->h_params[c].fm_k;
        e->h_params[c].wbfm_k_prev = e->h_params[c].wbfm_k;
        e->h_params[c].fm_k_prev = e->h_params[c].fm_k;
        e->h_params[c].k_changed = 0;
        e->h_params[c].rotation_prev = e->h_params[c].rotation;
    }
    e->rot_applied.resize(e->n_ch);
    for (uint32_t c = 0; c < e->n_ch; c++) e->rot_applied[c] = e->h_params[c].rotation;
    // FrequencyScanner constructor defaults (FrequencyScanner.cc:96-131)
    ScanConfig sc0{};
    sc0.start_hz = sc0.end_hz = 162550000ull;
    e->h_scan.assign(e->n_ch, sc0);
    e->scan_new_cfg.assign(e->n_ch, 0);
    ScanState ss0{162550000ull, 0ull};
    std::vector<ScanState> scan_states(e->n_ch, ss0);

    std::vector<float> atan_lut, fm_lut;
    build_atan2_lut(atan_lut);
    build_fm_lut(fm_lut);
    std::vector<float> half_lut((size_t)129 * ST_ROW_FLOATS);
    e->stream_ok = build_half_lut(half_lut.data());
    e->knobs.stream_ok = e->stream_ok;
    std::vector<uint32_t> amat[3];
    {
        int16_t pre[16];
        quantize_q15(taps::WBFM_PRE, 16, pre);
        for (int r = 0; r < 3; r++) {
            amat[r].assign(8 * 64 * 4, 0u);
            build_stream_amat(r - 1, pre, amat[r].data());
        }
    }
    std::vector<uint32_t> amat4((size_t)2 * 3 * 4 * 64 * 4, 0u);
    for (int r = 0; r < 3; r++) {
        build_decim4_amat(r - 1, e->consts.fm_tuner, 32, amat4.data() + (size_t)r * 4 * 64 * 4);
        build_decim4_amat(r - 1, e->consts.am_s1, 8, amat4.data() + (size_t)(3 + r) * 4 * 64 * 4);
    }
    build_d4_taps(e->consts, e->d4_args);
    e->fm_kmax.resize(e->n_ch);
    for (uint32_t c = 0; c < e->n_ch; c++) e->fm_kmax[c] = fabsf(e->h_params[c].fm_k);
    build_stream_taps(e->consts.wbfm_d1, e->consts.post12, e->consts.audio40, e->stream_args);
    e->stream_args.b0 = e->consts.deemph_b0;
    e->stream_args.a1 = e->consts.deemph_a1;
    e->wbfm_kmax.resize(e->n_ch);
    for (uint32_t c = 0; c < e->n_ch; c++) e->wbfm_kmax[c] = fabsf(e->h_params[c].wbfm_k);

    const size_t n = e->n_ch;
    bool ok = hipStreamCreateWithFlags(e->stream.put(), hipStreamNonBlocking) == hipSuccess;
    {
        static std::mutex attr_mu;   // engines may be created from several threads
        std::lock_guard<std::mutex> lk(attr_mu);
        ok = ok && init_wbfm_stream_kernels() == hipSuccess && init_d4_stream_kernels() == hipSuccess && init_mixed_stream_kernels() == hipSuccess;
    }
    ok = ok && e->d_params.alloc(n) == hipSuccess;
    ok = ok && e->d_tails.alloc(n * FAM_COUNT * TAIL_BYTES) == hipSuccess;
    ok = ok && e->d_wcarry.alloc(n) == hipSuccess;
    ok = ok && e->d_dc.alloc(n * 2) == hipSuccess;
    ok = ok && e->d_tracker.alloc(n) == hipSuccess;
    ok = ok && e->d_agc_cfg.alloc(n) == hipSuccess;
    ok = ok && e->d_agc.alloc(n) == hipSuccess;
    ok = ok && e->d_epochs.alloc(n) == hipSuccess;
    ok = ok && e->d_scan_cfg.alloc(n) == hipSuccess;
    ok = ok && e->d_scan.alloc(n) == hipSuccess;
    ok = ok && e->d_atan.alloc(atan_lut.size()) == hipSuccess;
    ok = ok && e->d_fmlut.alloc(fm_lut.size()) == hipSuccess;
    ok = ok && e->d_half_lut.alloc(half_lut.size()) == hipSuccess;
    for (int r = 0; r < 3; r++) ok = ok && e->d_amat[r].alloc(amat[r].size()) == hipSuccess;
    ok = ok && e->d_amat4.alloc(amat4.size()) == hipSuccess;
    ok = ok && e->d_counters.alloc(CNT_COUNT) == hipSuccess;
    ok = ok && hipMemset(e->d_counters, 0, CNT_COUNT * sizeof(uint32_t)) == hipSuccess;
    ok = ok && e->d_stamps.alloc(32768) == hipSuccess;
    ok = ok && hipMemset(e->d_stamps, 0, 32768 * sizeof(unsigned long long)) == hipSuccess;
    ok = ok && e->h_counters.alloc(CNT_COUNT) == hipSuccess;
    if (ok) {
        ok = hipMemsetAsync(e->d_tails, 0x80, n * FAM_COUNT * TAIL_BYTES, e->stream) == hipSuccess;
        ok = ok && hipMemsetAsync(e->d_wcarry, 0, n * sizeof(WbfmCarry), e->stream) == hipSuccess;
        ok = ok && hipMemsetAsync(e->d_dc, 0, n * 2 * sizeof(DcCarry), e->stream) == hipSuccess;
        ok = ok && hipMemsetAsync(e->d_tracker, 0, n * sizeof(uint32_t), e->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(e->d_agc, agc_states.data(), n * sizeof(AgcState), hipMemcpyHostToDevice,
                                  e->stream) == hipSuccess;
        ok = ok && hipMemsetAsync(e->d_epochs, 0x7f, n * sizeof(GainEpoch), e->stream) == hipSuccess;   // "long ago"
        ok = ok && hipMemcpyAsync(e->d_scan, scan_states.data(), n * sizeof(ScanState), hipMemcpyHostToDevice,
                                  e->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(e->d_atan, atan_lut.data(), atan_lut.size() * sizeof(float),
                                  hipMemcpyHostToDevice, e->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(e->d_fmlut, fm_lut.data(), fm_lut.size() * sizeof(float),
                                  hipMemcpyHostToDevice, e->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(e->d_half_lut, half_lut.data(), half_lut.size() * sizeof(float),
                                  hipMemcpyHostToDevice, e->stream) == hipSuccess;
        for (int r = 0; r < 3; r++)
            ok = ok && hipMemcpyAsync(e->d_amat[r], amat[r].data(), amat[r].size() * sizeof(uint32_t),
                                      hipMemcpyHostToDevice, e->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync(e->d_amat4, amat4.data(), amat4.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                  e->stream) == hipSuccess;
        ok = ok && upload_consts(e->consts, e->stream) == hipSuccess;
        ok = ok && hipStreamSynchronize(e->stream) == hipSuccess;
    }
    if (!ok) {
        iqd_destroy(e);
        return IQD_ENOMEM;
    }
    *out = e;
    return IQD_OK;
}

void iqd_destroy(iqd_t *e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    // nothing is released while a stream may still run; the members release themselves
    for (hipStream_t st : {e->stream.get(), e->pre_stream.get(), e->copy_stream.get(), e->fam_stream[0].get(), e->fam_stream[1].get(), e->fam_stream[2].get()})
        if (st) (void)hipStreamSynchronize(st);
    delete e;
}

int iqd_set_mode(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int mode)
{
    if (!range_ok(e, first_ch, n_ch) || mode < IQD_MODE_NONE || mode > IQD_MODE_USB) return IQD_EINVAL;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->mode_gen.size() < e->h_params.size()) e->mode_gen.resize(e->h_params.size(), 0u);
    for (uint32_t c = first_ch; c < first_ch + n_ch; c++) {
        e->h_params[c].mode = mode;
        e->mode_gen[c]++;
        if (mode == IQD_MODE_LSB) e->h_params[c].ssb_lsb = 1;  // IqDataProcessor.cc:244-256
        if (mode == IQD_MODE_USB) e->h_params[c].ssb_lsb = 0;
    }
    e->params_dirty = e->lists_dirty = true;
    return IQD_OK;
}

int iqd_set_gain(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int demod, float gain)
{
    if (!range_ok(e, first_ch, n_ch) || demod < IQD_DEMOD_AM || demod > IQD_DEMOD_SSB) return IQD_EINVAL;
    static const int fam[5] = {0, FAM_AM, FAM_FM, FAM_WBFM, FAM_SSB};
    std::lock_guard<std::mutex> lk(e->mu);
    for (uint32_t c = first_ch; c < first_ch + n_ch; c++) {
        e->h_params[c].gain[fam[demod]] = gain;
        derive_params(e->h_params[c]);
        const float ak = fabsf(e->h_params[c].wbfm_k), fk = fabsf(e->h_params[c].fm_k);
        if (!(ak <= e->wbfm_kmax[c])) e->wbfm_kmax[c] = ak;   // (NaN included: never "bounded" again)
        if (!(fk <= e->fm_kmax[c])) e->fm_kmax[c] = fk;
    }
    e->params_dirty = true;
    return IQD_OK;
}

int iqd_set_squelch(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int32_t threshold)
{
    if (!range_ok(e, first_ch, n_ch)) return IQD_EINVAL;
    std::lock_guard<std::mutex> lk(e->mu);
    for (uint32_t c = first_ch; c < first_ch + n_ch; c++) e->h_params[c].threshold = threshold;
    e->params_dirty = e->lists_dirty = true;
    return IQD_OK;
}

int iqd_set_rx_gain_db(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint32_t gain_db)
{
    if (!range_ok(e, first_ch, n_ch)) return IQD_EINVAL;
    std::lock_guard<std::mutex> lk(e->mu);
    for (uint32_t c = first_ch; c < first_ch + n_ch; c++) {
        e->h_params[c].rx_gain_db = gain_db;
        e->h_agc[c].set_gain = gain_db;                      // the device holds the gain in force
        if (!e->h_agc[c].enabled) e->agc_touched[c] = 0;     // and nothing there will move it
    }
    e->params_dirty = e->lists_dirty = e->agc_dirty = true;
    return IQD_OK;
}

// ---- AutomaticGainControl: the reference's setters one to one (they validate like the reference does) ----
extern "C++" {
template <class F>
static int agc_update(iqd_t *e, uint32_t first_ch, uint32_t n_ch, bool valid, F f)
{
    if (!range_ok(e, first_ch, n_ch)) return IQD_EINVAL;
    if (!valid) return e->fail(IQD_EINVAL, "AGC parameter out of range");
    std::lock_guard<std::mutex> lk(e->mu);
    for (uint32_t c = first_ch; c < first_ch + n_ch; c++) f(e->h_agc[c], c);
    e->agc_dirty = e->lists_dirty = true;
    return IQD_OK;
}
}  // extern "C++"

int iqd_agc_set_type(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint32_t type)
{
    return agc_update(e, first_ch, n_ch, type == IQD_AGC_LOWPASS || type == IQD_AGC_HARRIS,
                      [&](AgcConfig &a, uint32_t) { a.type = type; });
}

int iqd_agc_set_deadband(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint32_t deadband_db)
{
    return agc_update(e, first_ch, n_ch, deadband_db <= 10, [&](AgcConfig &a, uint32_t) { a.deadband = (int32_t)deadband_db; });
}

int iqd_agc_set_blanking_limit(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint32_t limit)
{
    return agc_update(e, first_ch, n_ch, limit <= 10, [&](AgcConfig &a, uint32_t) {
        a.blanking_limit = limit;
        a.reset_blanking = 1;   // setBlankingLimit() also resets the blanking system
    });
}

int iqd_agc_set_operating_point(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int32_t dbfs)
{
    return agc_update(e, first_ch, n_ch, true, [&](AgcConfig &a, uint32_t) { a.operating_point = dbfs; });
}

int iqd_agc_set_filter_coefficient(iqd_t *e, uint32_t first_ch, uint32_t n_ch, float coefficient)
{
    // the reference compares the float against double literals
    return agc_update(e, first_ch, n_ch, (coefficient >= 0.001) && (coefficient < 0.999),
                      [&](AgcConfig &a, uint32_t) { a.alpha = coefficient; });
}

int iqd_agc_enable(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int enabled)
{
    uint32_t changed = 0;
    int rc = agc_update(e, first_ch, n_ch, true, [&](AgcConfig &a, uint32_t c) {
        if (enabled && !a.enabled) {
            a.reset_blanking = 1;   // enable() of a disabled AGC resets the blanking system
            a.enabled = 1;
            e->agc_touched[c] = 1;
            changed++;
        } else if (!enabled && a.enabled) {
            a.enabled = 0;
            changed++;
        }
    });
    if (rc == IQD_OK && !changed) return IQD_EALREADY;   // enable()/disable() return false
    return rc;
}

extern "C++" {
// Uploads the channel parameters if they changed.  A WBFM / FM gain that differs from what the device last ran with
// hands the old K over for the histories (GainEpoch); agc_sync() then applies and clears the flags.  Call with e->mu held.
int iqd::upload_params(iqd_t *e)
{
    if (!e->params_dirty) return IQD_OK;
    for (uint32_t c = 0; c < e->n_ch; c++) {
        ChanParams &p = e->h_params[c];
        // (a change still pending - uploaded by a front-end call, not yet applied by agc_sync - keeps ITS "before":
        // the histories on the device were made with that one, whatever the value was set to in between)
        if (f2u(p.wbfm_k) != f2u(e->k_applied[2 * c])) {
            if (!(p.k_changed & 1u)) p.wbfm_k_prev = e->k_applied[2 * c];
            p.k_changed |= 1u;
            e->k_applied[2 * c] = p.wbfm_k;
            if (!e->wbfm_epoch_left[c]) e->wbfm_epochs_live++;
            e->wbfm_epoch_left[c] = (uint32_t)TAIL;
            e->wbfm_epoch_seq[c] = e->accept_seq + 1;
        } else if (!e->wbfm_epoch_left[c] && e->wbfm_kmax[c] < iqd_engine::WBFM_KMAX_DECAYS) {
            e->wbfm_kmax[c] = fabsf(p.wbfm_k);   // (a gain set and set back before any call ran with it: no change, no epoch to age it out)
        }
        if (f2u(p.fm_k) != f2u(e->k_applied[2 * c + 1])) {
            if (!(p.k_changed & 2u)) p.fm_k_prev = e->k_applied[2 * c + 1];
            p.k_changed |= 2u;
            e->k_applied[2 * c + 1] = p.fm_k;
        }
        if (p.rotation != e->rot_applied[c]) {
            if (!(p.k_changed & 4u)) p.rotation_prev = e->rot_applied[c];
            p.k_changed |= 4u;
            e->rot_applied[c] = p.rotation;
            e->rot_changed = true;
        }
        if (p.k_changed) e->agc_dirty = true;
    }
    HIP_TRY(e, hipMemcpyAsync(e->d_params, e->h_params.data(), e->n_ch * sizeof(ChanParams), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));  // the mirror may change once the lock is dropped
    e->params_dirty = false;
    return IQD_OK;
}

// Uploads the AGC configuration and applies the pending one-shot commands.  Call with e->mu held.
int iqd::agc_sync(iqd_t *e)
{
    if (!e->agc_dirty) return IQD_OK;
    hipStream_t s = e->stream;
    HIP_TRY(e, hipMemcpyAsync(e->d_agc_cfg, e->h_agc.data(), e->n_ch * sizeof(AgcConfig), hipMemcpyHostToDevice, s));
    HIP_TRY(e, hipMemcpyAsync(e->d_scan_cfg, e->h_scan.data(), e->n_ch * sizeof(ScanConfig), hipMemcpyHostToDevice, s));
    if (e->rot_changed) {   // before the flags are cleared: rewrite the tails of the channels whose rotation changed
        HIP_TRY(e, launch_retail(e->d_tails, e->d_params, e->n_ch, s));
        e->rot_changed = false;
    }
    HIP_TRY(e, launch_agc_apply(e->d_agc_cfg, e->d_agc, e->d_scan_cfg, e->d_scan, e->d_params, e->d_epochs, e->n_ch, s));
    HIP_TRY(e, hipStreamSynchronize(s));
    for (auto &a : e->h_agc) { a.reset_blanking = 0; a.set_gain = 0xffffffffu; }
    for (auto &c : e->h_scan) c.set_current_flag = 0;
    for (auto &p : e->h_params) p.k_changed = 0;   // (the kernel cleared the device copies)
    e->agc_dirty = false;
    return IQD_OK;
}
}  // extern "C++"

int iqd_agc_get_state(iqd_t *e, uint32_t ch, iqd_agc_state *out)
{
    if (!e || ch >= e->n_ch || !out) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    AgcState st;
    AgcConfig cfg;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        int rc = agc_sync(e);
        if (rc != IQD_OK) return rc;
        cfg = e->h_agc[ch];
    }
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(&st, e->d_agc + ch, sizeof(st), hipMemcpyDeviceToHost));
    out->enabled = cfg.enabled; out->type = cfg.type; out->operating_point_dbfs = cfg.operating_point;
    out->deadband_db = (uint32_t)cfg.deadband; out->blanking_limit = cfg.blanking_limit; out->alpha = cfg.alpha;
    out->rx_gain_db = st.rx_gain; out->if_gain_db = st.if_gain; out->filtered_if_gain_db = st.filtered;
    out->blanking_counter = st.blank_ctr; out->gain_was_adjusted = st.adjusted;
    out->normalized_level_dbfs = st.normalized; out->signal_magnitude = st.signal_magnitude;
    return IQD_OK;
}

int iqd_get_rx_gain_db(iqd_t *e, uint32_t ch, uint32_t *gain_db)
{
    iqd_agc_state st;
    if (!gain_db) return IQD_EINVAL;
    int rc = iqd_agc_get_state(e, ch, &st);
    if (rc == IQD_OK) *gain_db = st.rx_gain_db;
    return rc;
}

// ---- FrequencyScanner: the reference's methods one to one -------------------------------------------
int iqd_scanner_set_parameters(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint64_t start_hz, uint64_t end_hz,
                               uint64_t increment_hz)
{
    if (!range_ok(e, first_ch, n_ch)) return IQD_EINVAL;
    std::lock_guard<std::mutex> lk(e->mu);
    uint32_t changed = 0;
    for (uint32_t c = first_ch; c < first_ch + n_ch; c++) {
        ScanConfig &sc = e->h_scan[c];
        if (sc.scanning) continue;           // setScanParameters() returns false while scanning
        sc.start_hz = start_hz; sc.end_hz = end_hz; sc.increment_hz = increment_hz;
        e->scan_new_cfg[c] = 1;
        changed++;
    }
    if (!changed) return IQD_EALREADY;
    e->agc_dirty = true;
    return IQD_OK;
}

int iqd_scanner_start(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int start)
{
    if (!range_ok(e, first_ch, n_ch)) return IQD_EINVAL;
    std::lock_guard<std::mutex> lk(e->mu);
    uint32_t changed = 0;
    for (uint32_t c = first_ch; c < first_ch + n_ch; c++) {
        ScanConfig &sc = e->h_scan[c];
        if (start && !sc.scanning) {
            if (e->scan_new_cfg[c]) {        // start(): jump to the end frequency and tune there
                sc.set_current = sc.end_hz;
                sc.set_current_flag = 1;
                e->scan_new_cfg[c] = 0;
            }
            sc.scanning = 1;
            changed++;
        } else if (!start && sc.scanning) {
            sc.scanning = 0;
            changed++;
        }
    }
    if (!changed) return IQD_EALREADY;       // start()/stop() return false
    e->agc_dirty = true;
    return IQD_OK;
}

int iqd_scanner_get(iqd_t *e, uint32_t ch, uint64_t *current_hz, uint64_t *tune_count, int *scanning)
{
    if (!e || ch >= e->n_ch) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    {
        std::lock_guard<std::mutex> lk(e->mu);
        int rc = agc_sync(e);
        if (rc != IQD_OK) return rc;
        if (scanning) *scanning = (int)e->h_scan[ch].scanning;
    }
    ScanState ss;
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(&ss, e->d_scan + ch, sizeof(ss), hipMemcpyDeviceToHost));
    if (current_hz) *current_hz = ss.current_hz;
    if (tune_count) *tune_count = ss.tune_count;
    return IQD_OK;
}

int iqd_get_frequency_trace(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint64_t *out, size_t n_blocks)
{
    if (!e || !out) return IQD_EINVAL;
    if (!e->trace_n || first_ch < e->trace_first || n_ch == 0 || first_ch + n_ch > e->trace_first + e->trace_n ||
        n_blocks != e->trace_blocks)
        return e->fail(IQD_EINVAL, "no frequency trace for that range (tracing on? same channels and block count as the last accept?)");
    (void)hipSetDevice(e->device);
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(out, e->freq_trace.as<unsigned long long>() + (size_t)(first_ch - e->trace_first) * n_blocks,
                         (size_t)n_ch * n_blocks * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return IQD_OK;
}

int iqd_set_gain_trace(iqd_t *e, int enabled)
{
    if (!e) return IQD_EINVAL;
    e->trace_on = enabled != 0;
    if (!e->trace_on) e->trace_n = 0;
    return IQD_OK;
}

int iqd_get_gain_trace(iqd_t *e, uint32_t first_ch, uint32_t n_ch, uint32_t *out, size_t n_blocks)
{
    if (!e || !out) return IQD_EINVAL;
    if (!e->trace_n || first_ch < e->trace_first || n_ch == 0 || first_ch + n_ch > e->trace_first + e->trace_n ||
        n_blocks != e->trace_blocks)
        return e->fail(IQD_EINVAL, "no gain trace for that range (tracing on? same channels and block count as the last accept?)");
    (void)hipSetDevice(e->device);
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(out, e->gain_trace.as<uint32_t>() + (size_t)(first_ch - e->trace_first) * n_blocks,
                         (size_t)n_ch * n_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return IQD_OK;
}

int iqd_set_rotation(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int rotation)
{
    if (!range_ok(e, first_ch, n_ch) || rotation < -1 || rotation > 1) return IQD_EINVAL;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->rot_gen.size() < e->h_params.size()) e->rot_gen.resize(e->h_params.size(), 0u);
    for (uint32_t c = first_ch; c < first_ch + n_ch; c++) {
        e->h_params[c].rotation = rotation;
        e->rot_gen[c]++;
    }
    e->params_dirty = e->lists_dirty = true;   // (the families' channel lists are grouped by selector for the streaming kernels)
    return IQD_OK;
}

int iqd_reset(iqd_t *e, uint32_t first_ch, uint32_t n_ch)
{
    if (!range_ok(e, first_ch, n_ch)) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    HIP_TRY(e, launch_reset(e->d_tails, e->d_wcarry, e->d_dc, first_ch, n_ch, 0xfu, e->stream));
    return IQD_OK;
}

int iqd_reset_demod(iqd_t *e, uint32_t first_ch, uint32_t n_ch, int demod)
{
    if (!range_ok(e, first_ch, n_ch) || demod < IQD_DEMOD_AM || demod > IQD_DEMOD_SSB) return IQD_EINVAL;
    static const int fam[5] = {0, FAM_AM, FAM_FM, FAM_WBFM, FAM_SSB};
    (void)hipSetDevice(e->device);
    HIP_TRY(e, launch_reset(e->d_tails, e->d_wcarry, e->d_dc, first_ch, n_ch, 1u << fam[demod], e->stream));
    return IQD_OK;
}

int iqd_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int iqd_get_device(iqd_t *e, int *device)
{
    if (!e || !device) return IQD_EINVAL;
    *device = e->device;
    return IQD_OK;
}

int iqd_get_channel_mode(iqd_t *e, uint32_t ch, int *mode)
{
    if (!e || ch >= e->n_ch || !mode) return IQD_EINVAL;
    std::lock_guard<std::mutex> lk(e->mu);
    *mode = e->h_params[ch].mode;
    return IQD_OK;
}

int iqd_get_channel_gain(iqd_t *e, uint32_t ch, int demod, float *gain)
{
    if (!e || ch >= e->n_ch || !gain || demod < IQD_DEMOD_AM || demod > IQD_DEMOD_SSB) return IQD_EINVAL;
    static const int fam[5] = {0, FAM_AM, FAM_FM, FAM_WBFM, FAM_SSB};
    std::lock_guard<std::mutex> lk(e->mu);
    *gain = e->h_params[ch].gain[fam[demod]];
    return IQD_OK;
}

int iqd_set_profiling(iqd_t *e, int enabled)
{
    if (!e) return IQD_EINVAL;
    e->profiling = enabled != 0;
    return IQD_OK;
}

int iqd_get_stats(iqd_t *e, iqd_stats *out)
{
    if (!e || !out) return IQD_EINVAL;
    // the verification / repair counters live on the device (accepts do not wait for them): wait and read
    (void)hipSetDevice(e->device);
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(e->h_counters, e->d_counters, CNT_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (auto &pr : e->ev_pending) {   // the stream is idle: every recorded pair has completed
        float ms = 0.f;
        HIP_TRY(e, hipEventElapsedTime(&ms, pr.first, pr.second));
        e->stats.chain_kernel_ms += ms;
        e->stats.chain_kernel_count++;
        e->ev_free_pairs.push_back(std::move(pr));
    }
    e->ev_pending.clear();
    e->stats.state_checks = e->h_counters[CNT_TILE_CHECKS] + e->stream_handoffs - e->h_counters[CNT_STREAM_MISMATCH];
    e->stats.segment_repairs = e->h_counters[CNT_SEG_REPAIRS];
    e->stats.state_repairs = (uint64_t)e->h_counters[CNT_TILE_REPAIRS] + e->h_counters[CNT_DC_REDO];
    *out = e->stats;
    return IQD_OK;
}

int iqd_synchronize(iqd_t *e)
{
    if (!e) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    return IQD_OK;
}

void *iqd_stream(iqd_t *e) { return e ? (void *)e->stream : nullptr; }

// Diagnostic builds (-DIQD_STAMPS) only: per-phase cycle sums of the chain kernel.
int iqd_debug_stamps(iqd_t *e, unsigned long long *out16)
{
    if (!e || !out16) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(out16, e->d_stamps, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return IQD_OK;
}

int iqd_debug_stamps_ext(iqd_t *e, unsigned long long *out, uint32_t n)
{
    if (!e || !out || n > 32768) return IQD_EINVAL;
    (void)hipSetDevice(e->device);
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    HIP_TRY(e, hipMemcpy(out, e->d_stamps, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return IQD_OK;
}

}  // extern "C"
