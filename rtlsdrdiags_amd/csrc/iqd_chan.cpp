// Wideband channelizer, host side (include/iqdemod.h: iqd_channelizer_*, iqd_accept_wideband): the object, its setters, the
// upload of its layout, run and accept_wideband.
//
// The layout (iqd_chan_layout.h) keeps the prototype, every channel's (source, increment, gain shift, kind) and complex taps,
// groups the channels into tiles of 8 and packs the tiles' taps as MFMA A operands; this file sends what changed through
// page-locked staging and queues the kernels on the engine's stream: chz_kernel (iqd_chan.hip) for the fixed channels, the
// walkers for those that follow their engine channel's IF gain (iqd_chan_gain.hip) or scanner, chz_track_kernel
// (iqd_chan_track.hip) for those that follow a slot of a track table.  Captures of a signed sample format (IQD_WIDE_S8,
// IQD_WIDE_S16) go to chz_fmt_kernel (iqd_chan_fmt.hip) with the same tiles and A operands; S16 adds the rows' coefficient sums.
// A call is a check with every refusal, a queue that refuses nothing and returns what the call would commit, and the commit;
// the host forms are staging around the same three.  The survey: iqd_chan_survey.cpp; the design: iqd_chan_design.cpp.
#include <algorithm>
#include <new>

#include "iqd_chan_impl.h"

using namespace iqd;

// ---- the object ---------------------------------------------------------------------------------------------------------------

static int chz_fill_history(iqd_channelizer *z)   // zero history: offset-binary 0x80; a signed format's raw bytes: 0
{
    const ChzGeometry &g = z->g;
    CHZ_TRY(z, hipMemsetAsync(z->d.hist[z->cur].p, g.fmt == IQD_WIDE_U8 ? 0x80 : 0, (size_t)g.n_src * 2 * g.kp * g.rail, z->stream));
    CHZ_TRY(z, hipMemsetAsync(z->track.carry[z->track.cur].p, 0, (size_t)g.n_ch * sizeof(uint2), z->stream));   // no carry is live
    z->m_abs = 0;
    return IQD_OK;
}

extern "C" {

int iqd_channelizer_create(iqd_t *e, const iqd_channelizer_config *cfg, iqd_channelizer_t **out)
{
    if (!e) return IQD_EINVAL;
    if (!cfg || !out) return engine_fail(e, IQD_EINVAL, "NULL config or output pointer");
    const uint32_t den = cfg->decimation_den ? cfg->decimation_den : 1;
    if (cfg->n_sources < 1 || cfg->n_channels < 1 || (den == 1 && (cfg->decimation < 2 || cfg->decimation > 64)))
        return engine_fail(e, IQD_EINVAL, "channelizer: n_sources, n_channels >= 1 and 2 <= decimation <= 64");
    if (!chz_ratio_ok(cfg->decimation, den))
        return engine_fail(e, IQD_EINVAL, "channelizer: decimation_den must be 0, 1, 2, 4 or 8, coprime to decimation, and 2 <= "
                                          "decimation / decimation_den <= 64");
    for (uint32_t r : cfg->reserved)
        if (r) return engine_fail(e, IQD_EINVAL, "channelizer: reserved fields must be 0");
    if (cfg->sample_format > IQD_WIDE_S16)
        return engine_fail(e, IQD_EINVAL, "channelizer: sample_format must be IQD_WIDE_U8, IQD_WIDE_S8 or IQD_WIDE_S16");
    if (cfg->sample_format != IQD_WIDE_U8 && den > 1)
        return engine_fail(e, IQD_EINVAL, cfg->sample_format == IQD_WIDE_S16
                               ? "channelizer: IQD_WIDE_S16 captures at a fractional rate (decimation_den > 1) are not built yet"
                               : "channelizer: IQD_WIDE_S8 captures at a fractional rate (decimation_den > 1) are not built yet");
    std::vector<int16_t> h;
    if (cfg->taps) {
        if (cfg->n_taps < 1 || cfg->n_taps > 1024 * den)
            return engine_fail(e, IQD_EINVAL, den == 1 ? "channelizer: 1 <= n_taps <= 1024" : "channelizer: 1 <= n_taps <= 1024 * decimation_den");
        h.assign(cfg->taps, cfg->taps + cfg->n_taps);
    } else {
        h.resize(iqd_channelizer_default_taps_q(cfg->decimation, den, nullptr, 0));
        iqd_channelizer_default_taps_q(cfg->decimation, den, h.data(), (uint32_t)h.size());
    }
    for (int16_t t : h)
        if (t > 32639 || t < -32639) return engine_fail(e, IQD_EINVAL, "channelizer: |h[k]| must be <= 32639");
    for (uint32_t br = 0; br < den; br++) {
        int64_t abs_sum = 0;
        for (size_t i = br; i < h.size(); i += den) abs_sum += h[i] < 0 ? -h[i] : h[i];
        if (256 * abs_sum > 2147483647LL - 255)
            return engine_fail(e, IQD_EINVAL, den == 1 ? "channelizer: 256 sum |h| must be <= 2^31 - 256"
                                                       : "channelizer: 256 sum |h| of every branch must be <= 2^31 - 256");
    }
    if (cfg->n_channels > (1u << 20) || cfg->n_sources > (1u << 20)) return engine_fail(e, IQD_EINVAL, "channelizer: too many channels or sources");

    iqd_channelizer *z = new (std::nothrow) iqd_channelizer;
    if (!z) return engine_fail(e, IQD_ENOMEM, "channelizer: host allocation failed");
    z->e = e;
    (void)iqd_get_device(e, &z->device);
    z->stream = (hipStream_t)iqd_stream(e);
    (void)hipSetDevice(z->device);
    z->g = ChzGeometry(*cfg, std::move(h));
    const ChzGeometry &g = z->g;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, z->device) == hipSuccess && cus > 0) z->g.n_cus = (uint32_t)cus;
    z->ch.create(g);
    z->centre.assign(g.n_src, 0);
    std::vector<uint32_t> packed(CHZ_PHASOR);
    for (uint32_t i = 0; i < CHZ_PHASOR; i++)
        packed[i] = (uint16_t)g.phasor[2 * i] | ((uint32_t)(uint16_t)g.phasor[2 * i + 1] << 16);
    const size_t hb = (size_t)g.n_src * 2 * g.kp * g.rail, cb = (size_t)g.n_ch * sizeof(uint2);
    bool ok = z->d.phasor.ensure(CHZ_PHASOR * 4) == hipSuccess && z->d.hist[0].ensure(hb) == hipSuccess &&
              z->d.hist[1].ensure(hb) == hipSuccess && z->track.carry[0].ensure(cb) == hipSuccess &&
              z->track.carry[1].ensure(cb) == hipSuccess;
    ok = ok && hipMemcpy(z->d.phasor.p, packed.data(), CHZ_PHASOR * 4, hipMemcpyHostToDevice) == hipSuccess;
    std::vector<int16_t> proto(g.kp, 0);
    if (g.q == 1) std::copy(g.h.begin(), g.h.end(), proto.begin());   // (the walker's; it does not run at q > 1)
    ok = ok && z->d.proto.ensure(g.kp * 2) == hipSuccess && z->d.centre.ensure((size_t)g.n_src * 8) == hipSuccess;
    ok = ok && hipMemcpy(z->d.proto.p, proto.data(), g.kp * 2, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && chz_fill_history(z) == IQD_OK && hipStreamSynchronize(z->stream) == hipSuccess;
    if (!ok) {
        iqd_channelizer_destroy(z);
        return engine_fail(e, IQD_ENOMEM, "channelizer: device allocation failed");
    }
    *out = z;
    return IQD_OK;
}

void iqd_channelizer_destroy(iqd_channelizer_t *z)
{
    if (!z) return;
    (void)hipSetDevice(z->device);
    (void)hipStreamSynchronize(z->stream);   // (the tap uploads' events lie on it)
    delete z;
}

int iqd_channelizer_reset(iqd_channelizer_t *z)
{
    if (!z) return IQD_EINVAL;
    (void)hipSetDevice(z->device);
    return chz_fill_history(z);
}

}  // extern "C"

// ---- the setters --------------------------------------------------------------------------------------------------------------

static bool chz_range_ok(uint32_t first, uint32_t n, uint32_t of) { return n >= 1 && first < of && n <= of - first; }

// Why a channel may not become of kind `want`, [want][obstacle]: the captures' format, a fractional rate, or the kind the
// channel is of already.  NULL: it may (a channel may always stop following: no row for CHZ_FIXED).
enum { CHZ_OB_S16, CHZ_OB_S8, CHZ_OB_FRAC, CHZ_OB_KIND /* + the kind */, CHZ_OBSTACLES = CHZ_OB_KIND + CHZ_KINDS };
static const char *const CHZ_KIND_REFUSAL[CHZ_KINDS][CHZ_OBSTACLES] = {
    {},
    {"channelizer: channels on IQD_WIDE_S16 captures cannot follow their gain yet",
     "channelizer: channels on IQD_WIDE_S8 captures cannot follow their gain yet",
     "channelizer: channels of a fractional channelizer (decimation_den > 1) cannot follow their gain yet", nullptr, nullptr,
     "channelizer: a channel that follows its scanner cannot follow its gain as well (not built yet)",
     "channelizer: a channel that follows a track slot cannot follow its scanner or its gain as well (not built yet)"},
    {"channelizer: channels on IQD_WIDE_S16 captures cannot follow a scanner yet",
     "channelizer: channels on IQD_WIDE_S8 captures cannot follow a scanner yet",
     "channelizer: channels of a fractional channelizer (decimation_den > 1) cannot follow a scanner", nullptr,
     "channelizer: a channel that follows its gain cannot follow its scanner as well (not built yet)", nullptr,
     "channelizer: a channel that follows a track slot cannot follow its scanner or its gain as well (not built yet)"},
    {"channelizer: channels on IQD_WIDE_S16 captures cannot follow tracks yet",
     "channelizer: channels on IQD_WIDE_S8 captures cannot follow tracks yet",
     "channelizer: channels of a fractional channelizer (decimation_den > 1) cannot follow tracks yet", nullptr,
     "channelizer: a channel that follows its gain cannot follow a track slot as well (not built yet)",
     "channelizer: a channel that follows its scanner cannot follow a track slot as well (not built yet)", nullptr},
};

// may channel c become of kind `want`?  The refusal's text, or NULL: yes
static const char *chz_kind_refusal(const iqd_channelizer *z, uint32_t c, int want)
{
    const int obstacle = z->g.fmt == IQD_WIDE_S16 ? CHZ_OB_S16 : z->g.fmt == IQD_WIDE_S8 ? CHZ_OB_S8 : z->g.q > 1 ? CHZ_OB_FRAC : CHZ_OB_KIND + z->ch.kind[c];
    return CHZ_KIND_REFUSAL[want][obstacle];
}

// channels [first, first + n) follow in the way of `kind` (a walker's), or stop doing so
static int chz_follow(iqd_channelizer *z, uint32_t first, uint32_t n, int follow, int kind)
{
    if (!chz_range_ok(first, n, z->g.n_ch)) return z->fail(IQD_EINVAL, "channelizer: bad channel range");
    for (uint32_t c = first; follow && c < first + n; c++)
        if (const char *why = chz_kind_refusal(z, c, kind)) return z->fail(IQD_EINVAL, why);
    for (uint32_t c = first; c < first + n; c++)
        if (follow || z->ch.kind[c] == kind) z->ch.set_kind(c, follow ? kind : CHZ_FIXED);
    return IQD_OK;
}

extern "C" {

int iqd_channelizer_set_channels(iqd_channelizer_t *z, uint32_t first, uint32_t n, const uint32_t *source,
                                 const uint32_t *phase_inc, const uint8_t *gain_shift)
{
    if (!z) return IQD_EINVAL;
    if (!chz_range_ok(first, n, z->g.n_ch)) return z->fail(IQD_EINVAL, "channelizer: bad channel range");
    for (uint32_t i = 0; i < n; i++) {
        if (source && source[i] >= z->g.n_src) return z->fail(IQD_EINVAL, "channelizer: source index out of range");
        if (gain_shift && gain_shift[i] > 8) return z->fail(IQD_EINVAL, "channelizer: gain shift must be 0..8");
    }
    ChzChannels &ch = z->ch;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = first + i;
        if (source && source[i] != ch.src[c]) {
            ch.src[c] = source[i];
            ch.layout_dirty = true;
        }
        if (gain_shift) ch.shift[c] = gain_shift[i];
        if (phase_inc) ch.inc[c] = phase_inc[i];
        ch.ch_dirty[c] = 1;
        ch.any_dirty = true;
        if (phase_inc) ch.new_taps(z->g, c);
    }
    return IQD_OK;
}

int iqd_channelizer_set_source_frequency(iqd_channelizer_t *z, uint32_t first_source, uint32_t n, const uint64_t *centre_hz)
{
    if (!z) return IQD_EINVAL;
    if (!centre_hz || !chz_range_ok(first_source, n, z->g.n_src)) return z->fail(IQD_EINVAL, "channelizer: bad source range");
    for (uint32_t i = 0; i < n; i++) z->centre[first_source + i] = centre_hz[i];
    z->centre_dirty = true;
    return IQD_OK;
}

int iqd_channelizer_follow_scanner(iqd_channelizer_t *z, uint32_t first, uint32_t n, int follow)
{
    return z ? chz_follow(z, first, n, follow, CHZ_SCAN) : IQD_EINVAL;
}

int iqd_channelizer_follow_gain(iqd_channelizer_t *z, uint32_t first, uint32_t n, int follow)
{
    return z ? chz_follow(z, first, n, follow, CHZ_GAIN) : IQD_EINVAL;
}

int iqd_channelizer_follow_tracks(iqd_channelizer_t *z, uint32_t first, uint32_t n, const int32_t *slot)
{
    if (!z) return IQD_EINVAL;
    if (!chz_range_ok(first, n, z->g.n_ch)) return z->fail(IQD_EINVAL, "channelizer: bad channel range");
    for (uint32_t i = 0; slot && i < n; i++) {
        if (slot[i] < -1 || slot[i] > 63) return z->fail(IQD_EINVAL, "channelizer: a track slot must be -1 or 0..63");
        if (slot[i] < 0) continue;
        if (const char *why = chz_kind_refusal(z, first + i, CHZ_TRACK)) return z->fail(IQD_EINVAL, why);
    }
    ChzChannels &ch = z->ch;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = first + i;
        const int32_t s = slot ? slot[i] : -1;
        if (s == ch.trk[c]) continue;
        if (s >= 0 || ch.kind[c] == CHZ_TRACK) ch.set_kind(c, s >= 0 ? CHZ_TRACK : CHZ_FIXED);
        ch.trk[c] = s;
        ch.trk_fresh[c] = s >= 0;   // a channel that starts to follow, or moves to another slot: its carry does not count
        ch.any_fresh = ch.any_fresh || s >= 0;
        ch.ch_dirty[c] = 1;
        ch.any_dirty = true;
    }
    return IQD_OK;
}

int iqd_channelizer_set_track_table(iqd_channelizer_t *z, const iqd_track_follow *t)
{
    if (!z) return IQD_EINVAL;
    if (!t) {
        z->track.table = iqd_track_follow{};
        return IQD_OK;
    }
    for (uint32_t r : t->reserved)
        if (r) return z->fail(IQD_EINVAL, "channelizer: a track table's reserved fields must be 0");
    if (t->n_slots < 1 || t->n_slots > 64) return z->fail(IQD_EINVAL, "channelizer: a track table's n_slots must be 1..64");
    if (t->n_blocks < 1) return z->fail(IQD_EINVAL, "channelizer: a track table's n_blocks must be >= 1");
    if (t->block_bytes == 0 || t->block_bytes % 64 != 0)
        return z->fail(IQD_EINVAL, "channelizer: a track table's block_bytes must be a positive multiple of 64");
    if (t->lag > 1) return z->fail(IQD_EINVAL, "channelizer: a track table's lag must be 0 or 1");
    if (t->min_state != IQD_TRACK_TENTATIVE && t->min_state != IQD_TRACK_ACTIVE)
        return z->fail(IQD_EINVAL, "channelizer: a track table's min_state must be IQD_TRACK_TENTATIVE (1) or IQD_TRACK_ACTIVE (2)");
    if (!t->slots_dev) return z->fail(IQD_EINVAL, "channelizer: a track table's slots_dev is NULL");
    if (((uintptr_t)t->slots_dev) & 15) return z->fail(IQD_EINVAL, "channelizer: a track table's slots_dev must be 16-byte aligned");
    z->track.table = *t;
    return IQD_OK;
}

}  // extern "C"

// ---- the upload ---------------------------------------------------------------------------------------------------------------

// Packs what changed (ChzLayout::repack) and queues its upload on the engine's stream; the channels are clean once all of it
// has been queued, not before.  No host synchronisation: the bytes go through page-locked staging.
static int chz_upload(iqd_channelizer *z)
{
    bool regrouped = false;
    const std::vector<ChzPiece> pieces = z->lay.repack(z->g, z->ch, &regrouped);
    for (int a = 0; regrouped && a < CHZ_ARRAYS; a++)   // (workgroup rows: one at least, so that the pointer is never NULL)
        CHZ_TRY(z, z->d.lay[a].ensure(a < CHZ_WGS ? z->lay.array(a).bytes : std::max(sizeof(ChzWg), z->lay.array(a).bytes)));
    std::vector<ChzStaging::Piece> copies;
    for (const ChzPiece &p : pieces)
        copies.push_back({z->d.lay[p.array].as<uint8_t>() + p.offset, (const uint8_t *)z->lay.array(p.array).p + p.offset, p.bytes});
    CHZ_TRY(z, z->upload(copies));
    z->ch.clean();
    return IQD_OK;
}

// ---- a call: check, queue, commit ---------------------------------------------------------------------------------------------

namespace iqd {

int chz_check_len(iqd_channelizer *z, size_t bytes_per_source)
{
    const ChzGeometry &g = z->g;
    if (g.fmt == IQD_WIDE_S16 && (bytes_per_source == 0 || bytes_per_source % (128 * (size_t)g.m) != 0))
        return z->fail(IQD_EINVAL, "channelizer: bytes_per_source of IQD_WIDE_S16 captures must be a positive multiple of 128 * decimation");
    if (bytes_per_source == 0 || bytes_per_source % (64 * (size_t)g.m) != 0)
        return z->fail(IQD_EINVAL, "channelizer: bytes_per_source must be a positive multiple of 64 * decimation");
    if (bytes_per_source / g.m * g.q > 0x7fffffffull) return z->fail(IQD_EINVAL, "channelizer: bytes_per_source too large");
    if (bytes_per_source > 0x7fffffffull) return z->fail(IQD_EINVAL, "channelizer: bytes_per_source too large");
    return IQD_OK;
}

// What every launch of one call shares: the capture, the history it starts from, the tables, the geometry.  The tiles and
// what goes out are the caller's (a.amat, a.tiles, a.wgs, a.out, a.out_row, a.hist_next).
ChzLaunch chz_launch(const iqd_channelizer *z, const void *wide_dev, size_t bytes_per_source)
{
    const ChzGeometry &g = z->g;
    ChzLaunch a{};
    a.wide = (const uint8_t *)wide_dev;
    a.hist = z->d.hist[z->cur].as<uint8_t>();
    a.phasor = z->d.phasor.as<uint32_t>();
    a.bytes_per_source = bytes_per_source;
    a.n_sources = g.n_src;
    a.n_out = (uint32_t)(g.row_bytes(bytes_per_source) / 2);   // a multiple of 32 q
    a.m = g.m;
    a.kp = g.kp;
    a.nq = g.nq;
    a.nbase = (uint32_t)(z->m_abs / g.q * g.m);   // m_abs is a multiple of 32 q
    a.den = g.q;
    a.rail_bytes = g.rail;
    a.t_blk = std::min(a.n_out, g.t_max());
    return a;
}

}  // namespace iqd

// the length rule, then every refusal of a call with track followers: no table, a slot the table does not have, the fit
static int chz_check_len_and_tracks(iqd_channelizer *z, size_t bytes_per_source)
{
    int rc = chz_check_len(z, bytes_per_source);
    if (rc != IQD_OK || !z->ch.n_kind[CHZ_TRACK]) return rc;
    const iqd_track_follow &t = z->track.table;
    if (!t.slots_dev) return z->fail(IQD_EINVAL, "channelizer: a channel follows a track slot and no track table is set");
    for (uint32_t c = 0; c < z->g.n_ch; c++)
        if (z->ch.trk[c] >= 0 && (uint32_t)z->ch.trk[c] >= t.n_slots)
            return z->fail(IQD_EINVAL, "channelizer: a channel follows a slot the track table does not have (slot >= n_slots)");
    if (z->g.row_bytes(bytes_per_source) != (size_t)t.n_blocks * t.block_bytes)
        return z->fail(IQD_EINVAL, "channelizer: with track followers bytes_per_source / decimation must be the table's n_blocks * block_bytes");
    return IQD_OK;
}

// what a queued call changes once it counts: applied by chz_commit, after everything of the call has been queued
struct ChzCommit {
    uint32_t n_out = 0;                           // outputs per channel
    bool track_ran = false;                       // the track kernel wrote the other carry
};

static void chz_commit(iqd_channelizer *z, const ChzCommit &c)
{
    z->cur ^= 1;
    z->m_abs += c.n_out;
    if (!c.track_ran) return;
    z->track.cur ^= 1;
    ChzChannels &ch = z->ch;
    if (ch.any_fresh) {   // the carries count from the next call on: those tiles are packed again
        for (uint32_t i = 0; i < z->g.n_ch; i++)
            if (ch.trk_fresh[i]) {
                ch.trk_fresh[i] = 0;
                ch.ch_dirty[i] = 1;
            }
        ch.any_fresh = false;
        ch.any_dirty = true;
    }
}

// chz_fmt_kernel's launch (a signed format: no following channels, no fractional rate - refused where they are asked for)
static ChzFmtLaunch chz_fmt_fill(const iqd_channelizer *z, const ChzLaunch &a)
{
    ChzFmtLaunch f{};
    f.a = a;
    f.gsum = z->d.lay[CHZ_GSUM].as<ChzFmtTile>();
    f.pstride = 2 * (a.t_blk * a.m + a.kp) + 16;
    return f;
}

// the gain walker's: the engine's state and the blocks are the scan walker's; b: its workgroups
static ChzGainLaunch chz_gain_fill(const iqd_channelizer *z, const ChzScanLaunch &scan, ChzLaunch &b)
{
    ChzGainLaunch gl{};
    static_cast<ChzWalkLaunch &>(gl) = scan;
    gl.waves = z->lay.wg[CHZ_GAIN].waves;
    gl.wpt = z->lay.wg[CHZ_GAIN].wpt;
    b.wgs = z->d.lay[CHZ_WGS + CHZ_GAIN].as<ChzWg>();
    return gl;
}

// chz_track_kernel's (the call has passed chz_check_len_and_tracks: the table is there and fits); b: its workgroups and window
static hipError_t chz_track_fill(iqd_channelizer *z, ChzLaunch &b, ChzTrackLaunch &t, uint32_t *run_blocks)
{
    const iqd_track_follow &table = z->track.table;
    t.slots = table.slots_dev;
    t.carry = z->track.carry[z->track.cur].as<uint2>();
    t.carry_next = z->track.carry[z->track.cur ^ 1].as<uint2>();
    t.proto = z->d.proto.as<int16_t>();
    t.n_slots = table.n_slots;
    t.n_blocks = table.n_blocks;
    t.block_out = table.block_bytes / 2;
    t.lag = table.lag;
    t.min_state = table.min_state;
    t.first_tile = z->lay.first_tile[CHZ_TRACK];
    t.n_tiles = z->lay.first_tile[CHZ_TRACK + 1] - t.first_tile;
    b.wgs = z->d.lay[CHZ_WGS + CHZ_TRACK].as<ChzWg>();
    b.t_blk = std::min(t.block_out, chz_track_window_outputs(z->g.m, z->g.kp));
    t.wins = (t.block_out + b.t_blk - 1) / b.t_blk;
    *run_blocks = t.n_blocks;
    if (z->g.nq <= CHZ_NQ_REG) return hipSuccess;
    // the scratch: CHZ_TRACK_SCRATCH bytes at most, or one block's operands
    const size_t per_block = (size_t)t.n_tiles * z->g.nq * 2 * 64 * 16;
    *run_blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>(t.n_blocks, CHZ_TRACK_SCRATCH / per_block));
    hipError_t err = z->track.amat.ensure(*run_blocks * per_block);
    t.amat = z->track.amat.as<uint4>();
    return err;
}

// Queues one checked call and refuses nothing: the upload of what changed, then chz_kernel for the fixed channels, the
// walkers for the following ones (scan != NULL; gain: its engine state and blocks are scan's), the track kernel, the history.
// *commit: what the call changes once the caller lets it count.
static int chz_queue(iqd_channelizer *z, const void *wide_dev, size_t bytes_per_source, void *out_dev, ChzScanLaunch *scan, ChzCommit *commit)
{
    (void)hipSetDevice(z->device);
    if (z->ch.any_dirty || z->ch.layout_dirty) {
        int rc = chz_upload(z);
        if (rc != IQD_OK) return rc;
    }
    ChzLaunch a = chz_launch(z, wide_dev, bytes_per_source);
    a.hist_next = z->d.hist[z->cur ^ 1].as<uint8_t>();
    a.amat = z->d.lay[CHZ_AMAT].as<uint4>();
    a.tiles = z->d.lay[CHZ_TILES].as<ChzTile>();
    a.wgs = z->d.lay[CHZ_WGS + CHZ_FIXED].as<ChzWg>();
    a.out = (uint8_t *)out_dev;
    a.out_row = 2 * a.n_out;
    commit->n_out = a.n_out;
    const ChzWgSet *wg = z->lay.wg;
    const uint32_t n_fixed = (uint32_t)wg[CHZ_FIXED].wgs.size();
    if (z->g.fmt != IQD_WIDE_U8) {
        CHZ_TRY(z, launch_channelizer_fmt(chz_fmt_fill(z, a), n_fixed, z->stream));
        return IQD_OK;
    }
    if (scan) {
        if (z->centre_dirty && z->ch.n_kind[CHZ_SCAN]) {   // (the scan walker's; the gain walker does not read them)
            CHZ_TRY(z, hipMemcpyAsync(z->d.centre.p, z->centre.data(), (size_t)z->g.n_src * 8, hipMemcpyHostToDevice, z->stream));
            CHZ_TRY(z, hipStreamSynchronize(z->stream));   // (the host vector may change once this returns)
            z->centre_dirty = false;
        }
        scan->proto = z->d.proto.as<int16_t>();
        scan->centre = z->d.centre.as<unsigned long long>();
        scan->t_blk = std::min(scan->block_out, z->g.t_max());   // the walkers' windows stay inside one block
        scan->waves = wg[CHZ_SCAN].waves;
        scan->wpt = wg[CHZ_SCAN].wpt;
    }
    if (scan && !wg[CHZ_GAIN].wgs.empty()) {   // before launch_channelizer: its history kernel comes last
        ChzLaunch b = a;
        const ChzGainLaunch gl = chz_gain_fill(z, *scan, b);
        CHZ_TRY(z, launch_channelizer_gain(b, (uint32_t)wg[CHZ_GAIN].wgs.size(), gl, z->stream));
    }
    commit->track_ran = !wg[CHZ_TRACK].wgs.empty();
    if (commit->track_ran) {
        ChzLaunch b = a;
        ChzTrackLaunch t{};
        uint32_t run_blocks = 0;
        CHZ_TRY(z, chz_track_fill(z, b, t, &run_blocks));
        CHZ_TRY(z, launch_channelizer_track(b, (uint32_t)wg[CHZ_TRACK].wgs.size(), t, run_blocks, z->stream));
    }
    CHZ_TRY(z, launch_channelizer(a, n_fixed, z->d.lay[CHZ_WGS + CHZ_SCAN].as<ChzWg>(), scan ? (uint32_t)wg[CHZ_SCAN].wgs.size() : 0u, scan, z->stream));
    return IQD_OK;
}

// ---- run ----------------------------------------------------------------------------------------------------------------------

static int run_check(iqd_channelizer *z, const void *wide, size_t bytes_per_source, const void *out, bool device)
{
    if (!wide || !out) return z->fail(IQD_EINVAL, "channelizer: NULL buffer");
    if (device && ((((uintptr_t)wide) | ((uintptr_t)out)) & 15)) return z->fail(IQD_EINVAL, "channelizer: buffers must be 16-byte aligned");
    if (z->ch.n_kind[CHZ_SCAN]) return z->fail(IQD_EINVAL, "channelizer: a channel follows its scanner; use iqd_accept_wideband*");
    if (z->ch.n_kind[CHZ_GAIN]) return z->fail(IQD_EINVAL, "channelizer: a channel follows its gain; use iqd_accept_wideband*");
    return chz_check_len_and_tracks(z, bytes_per_source);
}

static int run_queue(iqd_channelizer *z, const void *wide_dev, size_t bytes_per_source, void *out_dev)
{
    ChzCommit commit;
    int rc = chz_queue(z, wide_dev, bytes_per_source, out_dev, nullptr, &commit);
    if (rc == IQD_OK) chz_commit(z, commit);
    return rc;
}

// ---- accept_wideband ----------------------------------------------------------------------------------------------------------

// one call's rows as the engine takes them: row bytes per channel, in nblk of its blocks (a short row: one)
struct WideGeometry { uint32_t e_nch = 0, bb = 0, flags = 0; size_t row = 0, nblk = 0; };
static WideGeometry wideband_geometry(const iqd_t *e, const iqd_channelizer *z, size_t bytes_per_source)
{
    WideGeometry w;
    engine_geometry(e, &w.e_nch, &w.bb, &w.flags);
    w.row = z->g.row_bytes(bytes_per_source);
    w.nblk = w.row % w.bb == 0 ? w.row / w.bb : 1;
    return w;
}

// every refusal of a wideband accept, in order; rows and the alignment are the device form's (the host form's rows are staging)
static int wideband_check(iqd_t *e, iqd_channelizer *z, uint32_t first_ch, const void *wide, size_t bytes_per_source, const void *rows,
                          const void *pcm, bool device)
{
    if (!z || z->e != e) return engine_fail(e, IQD_EINVAL, "accept_wideband: the channelizer belongs to another engine");
    if (!wide || !rows || !pcm) return z->fail(IQD_EINVAL, "accept_wideband: NULL buffer");
    if (device && ((((uintptr_t)wide) | ((uintptr_t)rows)) & 15)) return z->fail(IQD_EINVAL, "accept_wideband: wide and rows buffers must be 16-byte aligned");
    int rc = chz_check_len_and_tracks(z, bytes_per_source);
    if (rc != IQD_OK) return rc;
    const WideGeometry w = wideband_geometry(e, z, bytes_per_source);
    if (first_ch >= w.e_nch || z->g.n_ch > w.e_nch - first_ch) return z->fail(IQD_EINVAL, "accept_wideband: bad engine channel range");
    if (w.row % w.bb != 0 && (w.row >= w.bb || w.row % 64 != 0))
        return z->fail(IQD_EINVAL, "accept_wideband: bytes_per_source / decimation must be a multiple of block_bytes, or one short block");
    return IQD_OK;
}

// Queues one checked wideband accept: the rows into rows_dev, then iqd_accept_iq_device on them.  With following channels
// the engine's pending settings are applied first (once), so that the walker reads the state the accept starts from.  The
// checks are the engine's own (range, block_bytes rule), so it does not refuse these rows; should it still, the channelizer
// commits nothing: the call's history went to the other buffer, so the stream stands where it stood, like the engine's.
static int wideband_queue(iqd_t *e, iqd_channelizer *z, uint32_t first_ch, const void *wide_dev, size_t bytes_per_source,
                          void *rows_dev, void *pcm_dev, void *pcm_count_dev, void *magnitude_dev, void *signal_present_dev)
{
    const WideGeometry w = wideband_geometry(e, z, bytes_per_source);
    (void)hipSetDevice(z->device);
    ChzScanLaunch sl{};
    const bool walkers = z->ch.n_kind[CHZ_SCAN] || z->ch.n_kind[CHZ_GAIN];
    if (walkers) {
        int rc = engine_settle(e, &sl);
        if (rc != IQD_OK) return rc;
        sl.first_ch = first_ch;
        sl.n_blocks = (uint32_t)w.nblk;
        sl.block_out = (uint32_t)(w.row / w.nblk / 2);
    }
    ChzCommit commit;
    int rc = chz_queue(z, wide_dev, bytes_per_source, rows_dev, walkers ? &sl : nullptr, &commit);
    if (rc != IQD_OK) return rc;
    if (w.flags & IQD_F_PREPASS_OVERLAP) CHZ_TRY(z, hipStreamSynchronize(z->stream));   // that path wants its input complete
    rc = iqd_accept_iq_device(e, first_ch, z->g.n_ch, rows_dev, w.row, pcm_dev, pcm_count_dev, magnitude_dev, signal_present_dev);
    if (rc == IQD_OK) chz_commit(z, commit);
    return rc;
}

extern "C" {

int iqd_channelizer_run_device(iqd_channelizer_t *z, const void *wide_dev, size_t bytes_per_source, void *out_dev)
{
    if (!z) return IQD_EINVAL;
    int rc = run_check(z, wide_dev, bytes_per_source, out_dev, true);
    return rc != IQD_OK ? rc : run_queue(z, wide_dev, bytes_per_source, out_dev);
}

int iqd_channelizer_run(iqd_channelizer_t *z, const uint8_t *wide, size_t bytes_per_source, uint8_t *out)
{
    if (!z) return IQD_EINVAL;
    int rc = run_check(z, wide, bytes_per_source, out, false);
    if (rc != IQD_OK) return rc;
    return chz_staged_call(z, {{wide, z->g.n_src * bytes_per_source, &z->stg.wide, CHZ_IN},
                               {out, z->g.n_ch * z->g.row_bytes(bytes_per_source), &z->stg.out, CHZ_OUT}},
                           [&] { return run_queue(z, z->stg.wide.p, bytes_per_source, z->stg.out.p); });
}

int iqd_accept_wideband_device(iqd_t *e, iqd_channelizer_t *z, uint32_t first_ch, const void *wide_dev, size_t bytes_per_source,
                               void *rows_dev, void *pcm_dev, void *pcm_count_dev, void *magnitude_dev, void *signal_present_dev)
{
    if (!e) return IQD_EINVAL;
    int rc = wideband_check(e, z, first_ch, wide_dev, bytes_per_source, rows_dev, pcm_dev, true);
    return rc != IQD_OK ? rc : wideband_queue(e, z, first_ch, wide_dev, bytes_per_source, rows_dev, pcm_dev, pcm_count_dev, magnitude_dev, signal_present_dev);
}

int iqd_accept_wideband(iqd_t *e, iqd_channelizer_t *z, uint32_t first_ch, const uint8_t *wide, size_t bytes_per_source,
                        int16_t *pcm, uint32_t *pcm_count, uint32_t *magnitude, uint8_t *signal_present)
{
    if (!e) return IQD_EINVAL;
    int rc = wideband_check(e, z, first_ch, wide, bytes_per_source, wide, pcm, false);
    if (rc != IQD_OK) return rc;
    const WideGeometry w = wideband_geometry(e, z, bytes_per_source);
    const size_t n = z->g.n_ch, row = w.row, nblk = w.nblk;
    return chz_staged_call(z, {{wide, z->g.n_src * bytes_per_source, &z->stg.wide, CHZ_IN}, {nullptr, n * row, &z->stg.rows, CHZ_OUT},
                               {pcm, n * (row / 64) * 2, &z->stg.pcm, CHZ_OUT}, {pcm_count, n * 4, &z->stg.cnt, CHZ_OUT},
                               {magnitude, n * nblk * 4, &z->stg.mag, CHZ_OUT}, {signal_present, n * nblk, &z->stg.sp, CHZ_OUT}},
                           [&] {
                               return wideband_queue(e, z, first_ch, z->stg.wide.p, bytes_per_source, z->stg.rows.p, z->stg.pcm.p, z->stg.cnt.p,
                                                     magnitude ? z->stg.mag.p : nullptr, signal_present ? z->stg.sp.p : nullptr);
                           });
}

}  // extern "C"
