// Wideband channelizer, host side (include/iqdemod.h: iqd_channelizer_*, iqd_accept_wideband).
//
// Keeps the prototype, every channel's (source, increment, gain shift) and complex taps, groups the channels by source
// into tiles of 8 (padding slots have zero taps and store nothing), packs the tiles' taps as MFMA A operands
// (iqd_chan.h) and queues the kernel of iqd_chan.hip on the engine's stream.  Only the channels a set_channels call
// names get new taps; the packing is redone at the next run.  Channels that follow their engine channel's IF gain
// (iqd_channelizer_follow_gain) get tiles and workgroups of their own and go to chz_gain_kernel (iqd_chan_gain.hip); so do
// channels that follow a slot of a track table (iqd_channelizer_follow_tracks; chz_track_kernel, iqd_chan_track.hip).  Captures of a signed sample format (IQD_WIDE_S8, IQD_WIDE_S16)
// go to chz_fmt_kernel (iqd_chan_fmt.hip) with the same tiles and A operands; S16 adds the rows' coefficient sums.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "iqdemod.h"
#include "iqd_chan.h"
#include "iqd_hipres.h"
#include "iqd_host.h"

using namespace iqd;

namespace {

// Page-locked staging of a tap upload: the copies read it after the host call returned, so a slot is refilled only once
// the event behind its last copies has passed (two slots: the wait is for the upload before the previous one).
struct Staging {
    PinnedArray<uint8_t> h;
    Event done;
    bool pending = false;
    hipError_t ensure(size_t bytes)
    {
        if (!done) {
            hipError_t e = hipEventCreateWithFlags(done.put(), hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        if (pending) {
            hipError_t e = hipEventSynchronize(done);
            if (e != hipSuccess) return e;
            pending = false;
        }
        return bytes <= h.n ? hipSuccess : h.alloc(bytes);
    }
    // the pieces through this slot to the device, queued on stream, and the event behind them
    struct Piece { void *dst; const void *src; size_t n; };
    hipError_t upload(const std::vector<Piece> &pieces, hipStream_t stream)
    {
        size_t bytes = 0, at = 0;
        for (const Piece &p : pieces) bytes += p.n;
        hipError_t e = ensure(bytes ? bytes : 16);
        for (const Piece &p : pieces) {
            if (e != hipSuccess) return e;
            memcpy(h + at, p.src, p.n);
            e = hipMemcpyAsync(p.dst, h + at, p.n, hipMemcpyHostToDevice, stream);
            at += p.n;
        }
        if (e == hipSuccess) e = hipEventRecord(done, stream);
        pending = e == hipSuccess;
        return e;
    }
};

// the four kinds of channel: each has tiles and workgroups of its own and its kernel
enum { CHZ_FIXED, CHZ_GAIN, CHZ_SCAN, CHZ_TRACK, CHZ_KINDS };
struct WgSet {
    std::vector<ChzWg> wgs;
    DevBufExact dev;
    uint32_t waves = 1, wpt = 1;                  // a walker's: tiles per workgroup, waves per tile
};

double bessel_i0(double x)
{
    double sum = 1, term = 1;
    for (int k = 1; k < 200; k++) {
        const double f = x / (2.0 * k);
        term *= f * f;
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

}  // namespace

struct iqd_channelizer {
    iqd_t *e = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t n_src = 0, n_ch = 0, m = 0, k = 0, kp = 0, nq = 0;
    uint32_t q = 1, kb = 0;                       // decimation m / q; kb = ceil(k / q), the longest branch
    uint32_t fmt = IQD_WIDE_U8, rail = 1;         // sample format of the captures; bytes per rail B (2: IQD_WIDE_S16)
    std::vector<int16_t> h, phasor;               // prototype [K]; (c, s) pairs [8192]
    std::vector<uint32_t> src, inc;
    std::vector<uint8_t> shift;
    std::vector<uint8_t> follow;                  // [n_ch]: the channel follows its engine channel's scanner
    std::vector<uint8_t> follow_gain;             // [n_ch]: the channel follows its engine channel's IF gain
    std::vector<unsigned long long> centre;       // [n_src]: source centre frequencies
    uint32_t n_follow = 0, n_gain = 0;
    std::vector<int32_t> trk;                     // [n_ch]: the table slot the channel follows, -1: none
    std::vector<uint8_t> trk_fresh;               // [n_ch]: it has started to follow since the last call (its carry does not count)
    uint32_t n_track = 0;
    bool any_fresh = false;
    iqd_track_follow table{};                     // the track table in force (slots_dev NULL: none)
    DevBufExact d_carry[2], d_track_amat;         // the followers' carries (live, d) [n_ch], by call parity; large K: the scratch
    int carry_cur = 0;
    bool track_ran = false;                       // the last queued call had track followers (wideband_queue's step back)
    bool centre_dirty = true;
    uint32_t n_cus = 256;
    std::vector<int16_t> gr, gi;                  // [n_ch][q branches][kb], zero from a branch's length on
    bool layout_dirty = true;                     // a channel changed source: regroup
    std::vector<uint8_t> ch_dirty;                // new taps since the last packing
    bool any_dirty = true;
    uint64_t m_abs = 0;                           // outputs per channel since create / reset
    std::vector<ChzTile> tiles;
    WgSet wg[CHZ_KINDS];                          // chz_kernel's workgroups (fixed channels), the gain walker's, the scan walker's, chz_track_kernel's
    uint32_t first_track_tile = 0;                // tiles [first_track_tile, tiles.size()) hold track followers
    uint32_t n_fixed_tiles = 0;                   // tiles [0, n_fixed_tiles) hold fixed channels,
    uint32_t n_packed_tiles = 0;                  // [n_fixed_tiles, n_packed_tiles) gain-following ones, then scanner-, then track-following
    std::vector<uint32_t> slot_of;                // [n_ch]: tile * 8 + slot
    std::vector<uint8_t> amat;                    // [n_tiles][q residues][nq][2][64][16]
    std::vector<ChzFmtTile> gsum;                 // [n_tiles]: the rows' coefficient sums (IQD_WIDE_S16 only)
    DevBufExact d_gsum;
    DevBufExact d_amat, d_tiles, d_phasor, d_proto, d_centre, d_hist[2], st_wide, st_out;
    DevBufExact w_rows, w_pcm, w_cnt, w_mag, w_sp;        // iqd_accept_wideband's device staging
    // the band survey: points measured on every source, in tiles of 8 of their own (iqd_chan_survey.hip)
    std::vector<uint32_t> sv_inc;
    std::vector<uint8_t> sv_shift;
    std::vector<ChzTile> sv_tiles;                // ch[l]: the point index
    std::vector<uint8_t> sv_amat;                 // [n_tiles][q residues][nq][2][64][16]
    bool sv_dirty = false;                        // packed, not uploaded yet
    DevBufExact d_sv_amat, d_sv_tiles, sv_mag;    // sv_mag: the host form's result
    Staging stg[2];                               // tap uploads
    int stg_cur = 0;
    int cur = 0;

    int fail(int code, const char *msg) { return engine_fail(e, code, msg); }
    // bytes of one channel's row for bytes_per_source capture bytes
    size_t row_bytes(size_t bytes_per_source) const { return bytes_per_source / ((size_t)m * rail) * q; }
};

#define CHZ_TRY(z, call)                                                                                  \
    do {                                                                                                  \
        hipError_t err_ = (call);                                                                         \
        if (err_ != hipSuccess) return (z)->fail(IQD_EHIP, hipGetErrorString(err_));                      \
    } while (0)

namespace iqd {

void chz_phasor_table(int16_t *out)
{
    for (int i = 0; i < (int)CHZ_PHASOR; i++) {
        const double ph = 2.0 * M_PI * i / CHZ_PHASOR;
        out[2 * i] = (int16_t)lrint(32767.0 * cos(ph));
        out[2 * i + 1] = (int16_t)lrint(32767.0 * sin(ph));
    }
}

void chz_channel_taps(const int16_t *h, uint32_t k, uint32_t inc, const int16_t *phasor, int16_t *gr, int16_t *gi)
{
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t i = (uint32_t)(j * inc) >> 20;
        gr[j] = (int16_t)(((int32_t)h[j] * phasor[2 * i] + (1 << 14)) >> 15);
        gi[j] = (int16_t)(((int32_t)h[j] * phasor[2 * i + 1] + (1 << 14)) >> 15);
    }
}

}  // namespace iqd

// complex taps of increment inc on every branch, gr / gi [q][kb]: branch r of the prototype is h_r[k] = h[k q + r],
// k < ceil((K - r) / q) (q = 1: the prototype itself)
static void chz_branch_taps(const iqd_channelizer *z, uint32_t inc, int16_t *gr, int16_t *gi)
{
    std::vector<int16_t> hr(z->kb);
    for (uint32_t r = 0; r < z->q; r++) {
        const uint32_t kr = z->k > r ? (z->k - r + z->q - 1) / z->q : 0;
        for (uint32_t k = 0; k < kr; k++) hr[k] = z->h[(size_t)k * z->q + r];
        chz_channel_taps(hr.data(), kr, inc, z->phasor.data(), gr + (size_t)r * z->kb, gi + (size_t)r * z->kb);
    }
}

static void chz_new_taps(iqd_channelizer *z, uint32_t c)
{
    const size_t at = (size_t)c * z->q * z->kb;
    chz_branch_taps(z, z->inc[c], &z->gr[at], &z->gi[at]);
    z->ch_dirty[c] = 1;
    z->any_dirty = true;
}

// channels sorted by source, 8 per tile, up to CHZ_WAVES tiles of one source per workgroup row; fixed, gain-following,
// scanner-following and track-following channels never share a tile.  A walker's workgroups take `waves` tiles each: as few as keep every CU
// busy; the rest of the workgroup's 8 waves share the tiles' outputs (wpt waves per tile).
static void chz_walker_wgs(const iqd_channelizer *z, const std::vector<ChzWg> &runs, WgSet &w)
{
    uint32_t n_tiles = 0;
    for (const ChzWg &r : runs) n_tiles += r.n_tiles;
    w.waves = std::max(1u, std::min(CHZ_WAVES, n_tiles / std::max(1u, z->n_cus)));
    w.wpt = 1;
    while (2 * w.wpt * w.waves <= CHZ_WAVES) w.wpt *= 2;
    for (const ChzWg &r : runs)
        for (uint32_t t = 0; t < r.n_tiles; t += w.waves)
            w.wgs.push_back(ChzWg{r.source, r.first_tile + t, std::min(w.waves, r.n_tiles - t), 0});
}

static void chz_group(iqd_channelizer *z)
{
    z->tiles.clear();
    for (WgSet &w : z->wg) w.wgs.clear();
    z->slot_of.assign(z->n_ch, 0);
    std::vector<std::vector<uint32_t>> by_src[CHZ_KINDS];
    for (auto &b : by_src) b.resize(z->n_src);
    for (uint32_t c = 0; c < z->n_ch; c++)
        by_src[z->follow[c] ? CHZ_SCAN : z->follow_gain[c] ? CHZ_GAIN : z->trk[c] >= 0 ? CHZ_TRACK : CHZ_FIXED][z->src[c]].push_back(c);
    std::vector<ChzWg> runs[CHZ_KINDS];           // following tiles per source
    for (int f = 0; f < CHZ_KINDS; f++) {
        if (f == CHZ_TRACK) z->first_track_tile = (uint32_t)z->tiles.size();
        for (uint32_t s = 0; s < z->n_src; s++) {
            const auto &list = by_src[f][s];
            const uint32_t first_tile = (uint32_t)z->tiles.size();
            for (size_t i = 0; i < list.size(); i += CHZ_TILE_CH) {
                ChzTile t;
                for (uint32_t l = 0; l < CHZ_TILE_CH; l++) {
                    t.ch[l] = i + l < list.size() ? list[i + l] : CHZ_NONE;
                    if (t.ch[l] != CHZ_NONE) z->slot_of[t.ch[l]] = (uint32_t)z->tiles.size() * CHZ_TILE_CH + l;
                }
                z->tiles.push_back(t);
            }
            const uint32_t n_tiles = (uint32_t)z->tiles.size() - first_tile;
            if (f == CHZ_FIXED || f == CHZ_TRACK)   // chz_kernel's geometry: rows of up to CHZ_WAVES tiles
                for (uint32_t t = 0; t < n_tiles; t += CHZ_WAVES)
                    z->wg[f].wgs.push_back(ChzWg{s, first_tile + t, std::min(CHZ_WAVES, n_tiles - t), 0});
            else if (n_tiles)
                runs[f].push_back(ChzWg{s, first_tile, n_tiles, 0});
        }
        if (f == CHZ_FIXED) z->n_fixed_tiles = (uint32_t)z->tiles.size();
        if (f == CHZ_GAIN) z->n_packed_tiles = (uint32_t)z->tiles.size();
    }
    chz_walker_wgs(z, runs[CHZ_GAIN], z->wg[CHZ_GAIN]);
    chz_walker_wgs(z, runs[CHZ_SCAN], z->wg[CHZ_SCAN]);
    z->amat.assign(z->tiles.size() * z->q * z->nq * 2 * 64 * 16, 0);
    if (z->fmt == IQD_WIDE_S16) z->gsum.assign(z->tiles.size(), ChzFmtTile{});
    std::fill(z->ch_dirty.begin(), z->ch_dirty.end(), 1);
}

// A operands of one tile slot (iqd_chan.h) into amat: rows 2 l (Ar) and 2 l + 1 (Ai), both planes, every K-chunk, for
// every output residue res (its branch: ((res + 1) m - 1) mod q).  gr / gi [q][kb]: the slot's taps, NULL = padding (zeros)
static void chz_pack_rows(const iqd_channelizer *z, uint8_t *amat, uint32_t tile, uint32_t l, const int16_t *gr, const int16_t *gi)
{
    for (uint32_t res = 0; res < z->q; res++) {
        const uint32_t br = (uint32_t)((((uint64_t)res + 1) * z->m - 1) % z->q);
        const size_t taps = (size_t)br * z->kb;
        for (uint32_t row = 0; row < 2; row++) {
            const uint32_t rho = 2 * l + row;
            for (uint32_t q = 0; q < z->nq; q++)
                for (uint32_t g = 0; g < 4; g++)
                    for (uint32_t j = 0; j < 16; j++) {
                        const uint32_t kappa = 64 * q + 16 * g + j, comp = kappa & 1;
                        const uint32_t kk = z->kp - 1 - kappa / 2;
                        int32_t v = 0;
                        if (gr && kk < z->kb) {
                            const int32_t r = gr[taps + kk], i = gi[taps + kk];
                            v = row == 0 ? (comp == 0 ? r : -i) : (comp == 0 ? i : r);
                        }
                        const int8_t lo = (int8_t)(v & 0xff);
                        const int8_t hi = (int8_t)((v - lo) / 256);
                        const size_t lane = rho + 16 * g;
                        for (uint32_t p = 0; p < 2; p++)
                            amat[(((((size_t)tile * z->q + res) * z->nq + q) * 2 + p) * 64 + lane) * 16 + j] =
                                (uint8_t)(p == 0 ? lo : hi);
                    }
        }
    }
}

static void chz_pack_slot(iqd_channelizer *z, uint32_t tile, uint32_t l)
{
    ChzTile &t = z->tiles[tile];
    const uint32_t c = t.ch[l];
    t.inc[l] = c == CHZ_NONE ? 0 : z->inc[c];
    t.shift[l] = c == CHZ_NONE ? 0 : z->shift[c];
    if (tile >= z->first_track_tile)         // a track follower: the slot it follows in the increment's place (iqd_chan.h)
        t.inc[l] = c == CHZ_NONE ? 0 : (uint32_t)z->trk[c] | (z->trk_fresh[c] ? CHZ_TRACK_FRESH : 0u);
    if (tile >= z->n_packed_tiles) return;   // a following channel whose kernel builds its operands itself, per block
    const size_t taps = c == CHZ_NONE ? 0 : (size_t)c * z->q * z->kb;
    chz_pack_rows(z, z->amat.data(), tile, l, c == CHZ_NONE ? nullptr : &z->gr[taps], c == CHZ_NONE ? nullptr : &z->gi[taps]);
    if (z->fmt == IQD_WIDE_S16) {   // the sums of rows 2 l (gr on I, -gi on Q) and 2 l + 1 (gi on I, gr on Q); |sum| < 2^25
        int32_t sr = 0, si = 0;
        for (uint32_t k = 0; c != CHZ_NONE && k < z->kb; k++) {
            sr += z->gr[taps + k];
            si += z->gi[taps + k];
        }
        z->gsum[tile].g[l][0] = sr - si;
        z->gsum[tile].g[l][1] = sr + si;
    }
}

// Packs the tiles that hold a channel with new parameters and queues their upload on the engine's stream (runs of
// consecutive such tiles as one copy each; after a regrouping, everything).  No host synchronisation: the bytes go
// through page-locked staging.
static int chz_upload(iqd_channelizer *z)
{
    const bool regroup = z->layout_dirty;
    if (regroup) chz_group(z);
    const size_t n_tiles = z->tiles.size(), tile_bytes = (size_t)z->q * z->nq * 2 * 64 * 16;
    std::vector<uint8_t> tile_dirty(n_tiles, regroup ? 1 : 0);
    for (uint32_t t = 0; t < n_tiles; t++)
        for (uint32_t l = 0; l < CHZ_TILE_CH; l++) {
            const uint32_t c = z->tiles[t].ch[l];
            if (regroup || (c != CHZ_NONE && z->ch_dirty[c])) {
                chz_pack_slot(z, t, l);
                tile_dirty[t] = 1;
            }
        }
    std::fill(z->ch_dirty.begin(), z->ch_dirty.end(), 0);
    if (regroup) {
        CHZ_TRY(z, z->d_amat.ensure(z->amat.size()));
        CHZ_TRY(z, z->d_tiles.ensure(n_tiles * sizeof(ChzTile)));
        if (z->fmt == IQD_WIDE_S16) CHZ_TRY(z, z->d_gsum.ensure(std::max<size_t>(1, n_tiles) * sizeof(ChzFmtTile)));
        for (WgSet &w : z->wg) CHZ_TRY(z, w.dev.ensure(std::max<size_t>(1, w.wgs.size()) * sizeof(ChzWg)));
    }
    std::vector<Staging::Piece> pieces;
    for (size_t t = 0; t < n_tiles; t++) {
        if (!tile_dirty[t]) continue;
        size_t n = 1;                             // a run of consecutive dirty tiles
        while (t + n < n_tiles && tile_dirty[t + n]) n++;
        const size_t na = t < z->n_packed_tiles ? std::min<size_t>(n, z->n_packed_tiles - t) : 0;
        if (na) pieces.push_back({z->d_amat.as<uint8_t>() + t * tile_bytes, &z->amat[t * tile_bytes], na * tile_bytes});
        pieces.push_back({z->d_tiles.as<ChzTile>() + t, &z->tiles[t], n * sizeof(ChzTile)});
        if (z->fmt == IQD_WIDE_S16) pieces.push_back({z->d_gsum.as<ChzFmtTile>() + t, &z->gsum[t], n * sizeof(ChzFmtTile)});
        t += n;                                   // (tile t + n is clean, or the end)
    }
    for (WgSet &w : z->wg)
        if (regroup && !w.wgs.empty()) pieces.push_back({w.dev.p, w.wgs.data(), w.wgs.size() * sizeof(ChzWg)});
    CHZ_TRY(z, z->stg[z->stg_cur].upload(pieces, z->stream));
    z->stg_cur ^= 1;
    z->layout_dirty = false;
    z->any_dirty = false;
    return IQD_OK;
}

static int chz_fill_history(iqd_channelizer *z)   // zero history: offset-binary 0x80; a signed format's raw bytes: 0
{
    CHZ_TRY(z, hipMemsetAsync(z->d_hist[z->cur].p, z->fmt == IQD_WIDE_U8 ? 0x80 : 0, (size_t)z->n_src * 2 * z->kp * z->rail, z->stream));
    CHZ_TRY(z, hipMemsetAsync(z->d_carry[z->carry_cur].p, 0, (size_t)z->n_ch * sizeof(uint2), z->stream));   // no carry is live
    z->m_abs = 0;
    return IQD_OK;
}

extern "C" {

int iqd_channelizer_phasor_table(int16_t out[8192])
{
    if (!out) return IQD_EINVAL;
    chz_phasor_table(out);
    return IQD_OK;
}

// Kaiser-windowed sinc (beta 5, cut-off 124 kHz at the wide rate, 13 M + 1 taps), quantised to Q15; the centre tap takes
// up the rounding so that the DC gain is exactly 32768.  Stopband from 156 kHz >= 53 dB, passband +-100 kHz ripple
// 0.32 dB (tests/test_chan_host.py checks the quantised taps for M in 2..64).
int iqd_channelizer_default_taps(uint32_t decimation, int16_t *out, uint32_t capacity)
{
    return iqd_channelizer_default_taps_q(decimation, 1, out, capacity);
}

// Q in {1, 2, 4, 8}, gcd(P, Q) = 1 (P odd when Q > 1), 2 <= P / Q <= 64
static bool chz_ratio_ok(uint32_t p, uint32_t q)
{
    if (q != 1 && q != 2 && q != 4 && q != 8) return false;
    if (q > 1 && p % 2 == 0) return false;
    return p >= 2 * q && p <= 64 * q;
}

// The same design at the rate 256000 P, quantised per branch r (taps r, r + Q, ...): each branch is normalised to DC gain
// 32768 on its own and its first largest tap takes up the rounding, so the gain does not ripple at the output rate.
int iqd_channelizer_default_taps_q(uint32_t decimation, uint32_t den, int16_t *out, uint32_t capacity)
{
    if (den == 0) den = 1;
    if (!chz_ratio_ok(decimation, den) || (!out && capacity)) return IQD_EINVAL;
    const uint32_t n = 13 * decimation + 1;
    const double fc = 124.0 / (256.0 * decimation), beta = 5.0, i0b = bessel_i0(beta);
    std::vector<double> w(n);
    for (uint32_t i = 0; i < n; i++) {
        const double x = (double)i - (n - 1) / 2.0, r = 2.0 * i / (n - 1) - 1.0;
        const double sinc = x == 0 ? 1.0 : sin(2 * M_PI * fc * x) / (2 * M_PI * fc * x);
        w[i] = 2 * fc * sinc * bessel_i0(beta * sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    }
    std::vector<int32_t> q(n);
    for (uint32_t br = 0; br < den; br++) {
        double sum = 0, peak = 0;
        for (uint32_t i = br; i < n; i += den) {
            sum += w[i];
            peak = std::max(peak, fabs(w[i]));
        }
        int32_t qs = 0;
        uint32_t at = br;                          // the first largest tap (two equal ones: a rounding apart at most)
        bool found = false;
        for (uint32_t i = br; i < n; i += den) {
            qs += q[i] = (int32_t)lrint(w[i] / sum * 32768.0);
            if (!found && fabs(w[i]) >= peak * (1 - 1e-12)) {
                at = i;
                found = true;
            }
        }
        q[at] += 32768 - qs;
    }
    for (uint32_t i = 0; i < n && i < capacity; i++) out[i] = (int16_t)q[i];
    return (int)n;
}

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
    z->n_src = cfg->n_sources;
    z->n_ch = cfg->n_channels;
    z->m = cfg->decimation;
    z->h = h;
    z->q = den;
    z->fmt = cfg->sample_format;
    z->rail = cfg->sample_format == IQD_WIDE_S16 ? 2 : 1;
    z->k = (uint32_t)h.size();
    z->kb = (z->k + den - 1) / den;
    z->kp = (z->kb + 31) / 32 * 32;
    z->nq = z->kp / 32;
    z->phasor.resize(2 * CHZ_PHASOR);
    chz_phasor_table(z->phasor.data());
    z->src.assign(z->n_ch, 0);
    z->inc.assign(z->n_ch, 0);
    z->shift.assign(z->n_ch, 0);
    z->follow.assign(z->n_ch, 0);
    z->follow_gain.assign(z->n_ch, 0);
    z->trk.assign(z->n_ch, -1);
    z->trk_fresh.assign(z->n_ch, 0);
    z->centre.assign(z->n_src, 0);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, z->device) == hipSuccess && cus > 0)
            z->n_cus = (uint32_t)cus;
    }
    z->gr.assign((size_t)z->n_ch * z->q * z->kb, 0);
    z->gi.assign((size_t)z->n_ch * z->q * z->kb, 0);
    z->ch_dirty.assign(z->n_ch, 0);
    for (uint32_t c = 0; c < z->n_ch; c++) chz_new_taps(z, c);
    std::vector<uint32_t> packed(CHZ_PHASOR);
    for (uint32_t i = 0; i < CHZ_PHASOR; i++)
        packed[i] = (uint16_t)z->phasor[2 * i] | ((uint32_t)(uint16_t)z->phasor[2 * i + 1] << 16);
    const size_t hb = (size_t)z->n_src * 2 * z->kp * z->rail;
    bool ok = z->d_phasor.ensure(CHZ_PHASOR * 4) == hipSuccess && z->d_hist[0].ensure(hb) == hipSuccess &&
              z->d_hist[1].ensure(hb) == hipSuccess && z->d_carry[0].ensure((size_t)z->n_ch * sizeof(uint2)) == hipSuccess &&
              z->d_carry[1].ensure((size_t)z->n_ch * sizeof(uint2)) == hipSuccess;
    ok = ok && hipMemcpy(z->d_phasor.p, packed.data(), CHZ_PHASOR * 4, hipMemcpyHostToDevice) == hipSuccess;
    std::vector<int16_t> proto(z->kp, 0);
    if (z->q == 1) std::copy(z->h.begin(), z->h.end(), proto.begin());   // (the walker's; it does not run at q > 1)
    ok = ok && z->d_proto.ensure(z->kp * 2) == hipSuccess && z->d_centre.ensure((size_t)z->n_src * 8) == hipSuccess;
    ok = ok && hipMemcpy(z->d_proto.p, proto.data(), z->kp * 2, hipMemcpyHostToDevice) == hipSuccess;
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

int iqd_channelizer_set_channels(iqd_channelizer_t *z, uint32_t first, uint32_t n, const uint32_t *source,
                                 const uint32_t *phase_inc, const uint8_t *gain_shift)
{
    if (!z) return IQD_EINVAL;
    if (n < 1 || first >= z->n_ch || n > z->n_ch - first) return z->fail(IQD_EINVAL, "channelizer: bad channel range");
    for (uint32_t i = 0; i < n; i++) {
        if (source && source[i] >= z->n_src) return z->fail(IQD_EINVAL, "channelizer: source index out of range");
        if (gain_shift && gain_shift[i] > 8) return z->fail(IQD_EINVAL, "channelizer: gain shift must be 0..8");
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = first + i;
        if (source && source[i] != z->src[c]) {
            z->src[c] = source[i];
            z->layout_dirty = true;
        }
        if (gain_shift) z->shift[c] = gain_shift[i];
        if (phase_inc) z->inc[c] = phase_inc[i];
        z->ch_dirty[c] = 1;
        z->any_dirty = true;
        if (phase_inc) chz_new_taps(z, c);
    }
    return IQD_OK;
}

static int chz_check_len(iqd_channelizer *z, size_t bytes_per_source)
{
    if (z->fmt == IQD_WIDE_S16 && (bytes_per_source == 0 || bytes_per_source % (128 * (size_t)z->m) != 0))
        return z->fail(IQD_EINVAL, "channelizer: bytes_per_source of IQD_WIDE_S16 captures must be a positive multiple of 128 * decimation");
    if (bytes_per_source == 0 || bytes_per_source % (64 * (size_t)z->m) != 0)
        return z->fail(IQD_EINVAL, "channelizer: bytes_per_source must be a positive multiple of 64 * decimation");
    if (bytes_per_source / z->m * z->q > 0x7fffffffull) return z->fail(IQD_EINVAL, "channelizer: bytes_per_source too large");
    if (bytes_per_source > 0x7fffffffull) return z->fail(IQD_EINVAL, "channelizer: bytes_per_source too large");
    return IQD_OK;
}

// every refusal of a call with track followers: no table, a slot the table does not have, the length rule
static int chz_check_tracks(iqd_channelizer *z, size_t bytes_per_source)
{
    if (!z->n_track) return IQD_OK;
    const iqd_track_follow &t = z->table;
    if (!t.slots_dev) return z->fail(IQD_EINVAL, "channelizer: a channel follows a track slot and no track table is set");
    for (uint32_t c = 0; c < z->n_ch; c++)
        if (z->trk[c] >= 0 && (uint32_t)z->trk[c] >= t.n_slots)
            return z->fail(IQD_EINVAL, "channelizer: a channel follows a slot the track table does not have (slot >= n_slots)");
    if (z->row_bytes(bytes_per_source) != (size_t)t.n_blocks * t.block_bytes)
        return z->fail(IQD_EINVAL, "channelizer: with track followers bytes_per_source / decimation must be the table's n_blocks * block_bytes");
    return IQD_OK;
}

// the most outputs of one window
static uint32_t chz_t_max(const iqd_channelizer *z) { return chz_window_outputs(z->m, z->kp, z->q, z->rail); }

// What every launch of one call shares: the capture, the history it starts from, the tables, the geometry.  The tiles and
// what goes out are the caller's (a.amat, a.tiles, a.wgs, a.out, a.out_row, a.hist_next).
static ChzLaunch chz_launch(const iqd_channelizer *z, const void *wide_dev, size_t bytes_per_source)
{
    ChzLaunch a{};
    a.wide = (const uint8_t *)wide_dev;
    a.hist = z->d_hist[z->cur].as<uint8_t>();
    a.phasor = z->d_phasor.as<uint32_t>();
    a.bytes_per_source = bytes_per_source;
    a.n_sources = z->n_src;
    a.n_out = (uint32_t)(z->row_bytes(bytes_per_source) / 2);   // a multiple of 32 q
    a.m = z->m;
    a.kp = z->kp;
    a.nq = z->nq;
    a.nbase = (uint32_t)(z->m_abs / z->q * z->m);   // m_abs is a multiple of 32 q
    a.den = z->q;
    a.rail_bytes = z->rail;
    a.t_blk = std::min(a.n_out, chz_t_max(z));
    return a;
}

// Queues one call: chz_kernel for the fixed channels, the walkers for the following ones (scan != NULL; gain: its
// engine state and blocks are scan's), the history.
static int chz_queue(iqd_channelizer *z, const void *wide_dev, size_t bytes_per_source, void *out_dev, ChzScanLaunch *scan)
{
    (void)hipSetDevice(z->device);
    if (z->any_dirty || z->layout_dirty) {
        int rc = chz_upload(z);
        if (rc != IQD_OK) return rc;
    }
    const uint32_t t_max = chz_t_max(z);
    ChzLaunch a = chz_launch(z, wide_dev, bytes_per_source);
    a.hist_next = z->d_hist[z->cur ^ 1].as<uint8_t>();
    a.amat = z->d_amat.as<uint4>();
    a.tiles = z->d_tiles.as<ChzTile>();
    a.wgs = z->wg[CHZ_FIXED].dev.as<ChzWg>();
    a.out = (uint8_t *)out_dev;
    a.out_row = 2 * a.n_out;
    const uint32_t n_fixed = (uint32_t)z->wg[CHZ_FIXED].wgs.size();
    if (scan) {
        if (z->centre_dirty && z->n_follow) {   // (the scan walker's; the gain walker does not read them)
            CHZ_TRY(z, hipMemcpyAsync(z->d_centre.p, z->centre.data(), (size_t)z->n_src * 8, hipMemcpyHostToDevice, z->stream));
            CHZ_TRY(z, hipStreamSynchronize(z->stream));   // (the host vector may change once this returns)
            z->centre_dirty = false;
        }
        scan->proto = z->d_proto.as<int16_t>();
        scan->centre = z->d_centre.as<unsigned long long>();
        scan->t_blk = scan->block_out <= t_max ? scan->block_out : t_max;   // the walkers' windows stay inside one block
    }
    if (z->fmt != IQD_WIDE_U8) {   // (no following channels, no fractional rate: refused where they are asked for)
        ChzFmtLaunch f{};
        f.a = a;
        f.gsum = z->d_gsum.as<ChzFmtTile>();
        f.pstride = 2 * (a.t_blk * a.m + a.kp) + 16;
        CHZ_TRY(z, launch_channelizer_fmt(f, n_fixed, z->stream));
    } else {
        const WgSet &gw = z->wg[CHZ_GAIN], &sw = z->wg[CHZ_SCAN];
        if (scan && !gw.wgs.empty()) {   // before launch_channelizer: its history kernel comes last
            ChzGainLaunch g{};
            static_cast<ChzWalkLaunch &>(g) = *scan;   // the engine's state and the blocks are the same
            g.waves = gw.waves;
            g.wpt = gw.wpt;
            ChzLaunch b = a;
            b.wgs = gw.dev.as<ChzWg>();
            CHZ_TRY(z, launch_channelizer_gain(b, (uint32_t)gw.wgs.size(), g, z->stream));
        }
        if (scan) {
            scan->waves = sw.waves;
            scan->wpt = sw.wpt;
        }
        const WgSet &tw = z->wg[CHZ_TRACK];
        z->track_ran = !tw.wgs.empty();
        if (z->track_ran) {   // (checked by chz_check_tracks: the table is there and fits the call)
            ChzTrackLaunch t{};
            t.slots = z->table.slots_dev;
            t.carry = z->d_carry[z->carry_cur].as<uint2>();
            t.carry_next = z->d_carry[z->carry_cur ^ 1].as<uint2>();
            t.proto = z->d_proto.as<int16_t>();
            t.n_slots = z->table.n_slots;
            t.n_blocks = z->table.n_blocks;
            t.block_out = z->table.block_bytes / 2;
            t.lag = z->table.lag;
            t.min_state = z->table.min_state;
            t.first_tile = z->first_track_tile;
            t.n_tiles = (uint32_t)z->tiles.size() - z->first_track_tile;
            ChzLaunch b = a;
            b.wgs = tw.dev.as<ChzWg>();
            b.t_blk = std::min(t.block_out, chz_track_window_outputs(z->m, z->kp));
            t.wins = (t.block_out + b.t_blk - 1) / b.t_blk;
            uint32_t run_blocks = t.n_blocks;
            if (z->nq > CHZ_NQ_REG) {   // the scratch: CHZ_TRACK_SCRATCH bytes at most, or one block's operands
                const size_t per_block = (size_t)t.n_tiles * z->nq * 2 * 64 * 16;
                run_blocks = (uint32_t)std::max<size_t>(1, std::min<size_t>(t.n_blocks, CHZ_TRACK_SCRATCH / per_block));
                CHZ_TRY(z, z->d_track_amat.ensure(run_blocks * per_block));
                t.amat = z->d_track_amat.as<uint4>();
            }
            CHZ_TRY(z, launch_channelizer_track(b, (uint32_t)tw.wgs.size(), t, run_blocks, z->stream));
            z->carry_cur ^= 1;
            if (z->any_fresh) {   // the carries count from the next call on: those tiles are packed again
                for (uint32_t c = 0; c < z->n_ch; c++)
                    if (z->trk_fresh[c]) {
                        z->trk_fresh[c] = 0;
                        z->ch_dirty[c] = 1;
                    }
                z->any_fresh = false;
                z->any_dirty = true;
            }
        }
        CHZ_TRY(z, launch_channelizer(a, n_fixed, sw.dev.as<ChzWg>(), scan ? (uint32_t)sw.wgs.size() : 0u, scan, z->stream));
    }
    z->cur ^= 1;
    z->m_abs += a.n_out;
    return IQD_OK;
}

int iqd_channelizer_run_device(iqd_channelizer_t *z, const void *wide_dev, size_t bytes_per_source, void *out_dev)
{
    if (!z) return IQD_EINVAL;
    if (!wide_dev || !out_dev) return z->fail(IQD_EINVAL, "channelizer: NULL buffer");
    if ((((uintptr_t)wide_dev) | ((uintptr_t)out_dev)) & 15) return z->fail(IQD_EINVAL, "channelizer: buffers must be 16-byte aligned");
    if (z->n_follow) return z->fail(IQD_EINVAL, "channelizer: a channel follows its scanner; use iqd_accept_wideband*");
    if (z->n_gain) return z->fail(IQD_EINVAL, "channelizer: a channel follows its gain; use iqd_accept_wideband*");
    int rc = chz_check_len(z, bytes_per_source);
    if (rc == IQD_OK) rc = chz_check_tracks(z, bytes_per_source);
    if (rc != IQD_OK) return rc;
    return chz_queue(z, wide_dev, bytes_per_source, out_dev, nullptr);
}

int iqd_channelizer_run(iqd_channelizer_t *z, const uint8_t *wide, size_t bytes_per_source, uint8_t *out)
{
    if (!z) return IQD_EINVAL;
    if (!wide || !out) return z->fail(IQD_EINVAL, "channelizer: NULL buffer");
    if (z->n_follow) return z->fail(IQD_EINVAL, "channelizer: a channel follows its scanner; use iqd_accept_wideband*");
    if (z->n_gain) return z->fail(IQD_EINVAL, "channelizer: a channel follows its gain; use iqd_accept_wideband*");
    int rc = chz_check_len(z, bytes_per_source);
    if (rc == IQD_OK) rc = chz_check_tracks(z, bytes_per_source);
    if (rc != IQD_OK) return rc;
    (void)hipSetDevice(z->device);
    const size_t ib = (size_t)z->n_src * bytes_per_source, ob = (size_t)z->n_ch * z->row_bytes(bytes_per_source);
    CHZ_TRY(z, z->st_wide.ensure(ib));
    CHZ_TRY(z, z->st_out.ensure(ob));
    CHZ_TRY(z, hipMemcpyAsync(z->st_wide.p, wide, ib, hipMemcpyHostToDevice, z->stream));
    rc = iqd_channelizer_run_device(z, z->st_wide.p, bytes_per_source, z->st_out.p);
    if (rc != IQD_OK) return rc;
    CHZ_TRY(z, hipMemcpyAsync(out, z->st_out.p, ob, hipMemcpyDeviceToHost, z->stream));
    CHZ_TRY(z, hipStreamSynchronize(z->stream));
    return IQD_OK;
}

int iqd_channelizer_set_survey(iqd_channelizer_t *z, uint32_t n_points, const uint32_t *phase_inc, const uint8_t *gain_shift)
{
    if (!z) return IQD_EINVAL;
    if (n_points > 4096) return z->fail(IQD_EINVAL, "channelizer: a survey has at most 4096 points");
    if (n_points && z->fmt != IQD_WIDE_U8)
        return z->fail(IQD_EINVAL, z->fmt == IQD_WIDE_S16 ? "channelizer: the band survey of IQD_WIDE_S16 captures is not built yet"
                                                          : "channelizer: the band survey of IQD_WIDE_S8 captures is not built yet");
    if (n_points && !phase_inc) return z->fail(IQD_EINVAL, "channelizer: NULL survey increments");
    for (uint32_t i = 0; gain_shift && i < n_points; i++)
        if (gain_shift[i] > 8) return z->fail(IQD_EINVAL, "channelizer: gain shift must be 0..8");
    z->sv_inc.assign(phase_inc, phase_inc + n_points);
    z->sv_shift.assign(n_points, 0);
    if (gain_shift) z->sv_shift.assign(gain_shift, gain_shift + n_points);
    const uint32_t n_tiles = (n_points + CHZ_TILE_CH - 1) / CHZ_TILE_CH;
    z->sv_tiles.assign(n_tiles, ChzTile{});
    z->sv_amat.assign((size_t)n_tiles * z->q * z->nq * 2 * 64 * 16, 0);
    std::vector<int16_t> gr((size_t)z->q * z->kb), gi((size_t)z->q * z->kb);
    for (uint32_t t = 0; t < n_tiles; t++)
        for (uint32_t l = 0; l < CHZ_TILE_CH; l++) {
            const uint32_t p = t * CHZ_TILE_CH + l;
            ChzTile &T = z->sv_tiles[t];
            T.ch[l] = p < n_points ? p : CHZ_NONE;
            T.inc[l] = p < n_points ? z->sv_inc[p] : 0;
            T.shift[l] = p < n_points ? z->sv_shift[p] : 0;
            if (p >= n_points) continue;                  // (padding: the zeros of assign)
            std::fill(gr.begin(), gr.end(), 0);
            std::fill(gi.begin(), gi.end(), 0);
            chz_branch_taps(z, T.inc[l], gr.data(), gi.data());
            chz_pack_rows(z, z->sv_amat.data(), t, l, gr.data(), gi.data());
        }
    z->sv_dirty = n_points != 0;
    return IQD_OK;
}

// the survey's point tiles to the device, through a staging slot like the channels' taps
static int chz_survey_upload(iqd_channelizer *z)
{
    const size_t ab = z->sv_amat.size(), tb = z->sv_tiles.size() * sizeof(ChzTile);
    CHZ_TRY(z, z->d_sv_amat.ensure(ab));
    CHZ_TRY(z, z->d_sv_tiles.ensure(tb));
    CHZ_TRY(z, z->stg[z->stg_cur].upload({{z->d_sv_amat.p, z->sv_amat.data(), ab}, {z->d_sv_tiles.p, z->sv_tiles.data(), tb}}, z->stream));
    z->stg_cur ^= 1;
    z->sv_dirty = false;
    return IQD_OK;
}

// every refusal of a survey that does not depend on the buffers
static int chz_survey_check(iqd_channelizer *z, size_t bytes_per_source, uint32_t block_bytes)
{
    if (z->sv_inc.empty()) return z->fail(IQD_EINVAL, "channelizer: no survey points set");
    if (z->n_follow) return z->fail(IQD_EINVAL, "channelizer: no survey while a channel follows its scanner");
    if (z->n_gain) return z->fail(IQD_EINVAL, "channelizer: no survey while a channel follows its gain");
    if (z->n_track) return z->fail(IQD_EINVAL, "channelizer: no survey while a channel follows a track slot");
    int rc = chz_check_len(z, bytes_per_source);
    if (rc != IQD_OK) return rc;
    const uint32_t unit = z->q > 1 ? 256 : 64;
    if (block_bytes == 0 || block_bytes % unit != 0 || block_bytes > (1u << 24))
        return z->fail(IQD_EINVAL, z->q > 1 ? "channelizer: a survey's block_bytes must be a multiple of 256, at most 2^24"
                                            : "channelizer: a survey's block_bytes must be a multiple of 64, at most 2^24");
    const size_t row = bytes_per_source / z->m * z->q;
    if (row % block_bytes != 0) return z->fail(IQD_EINVAL, "channelizer: a survey's block_bytes must divide the row length");
    const uint64_t n_res = (uint64_t)z->n_src * (row / block_bytes) * z->sv_inc.size();
    const uint32_t n_out = (uint32_t)(row / 2), t_blk = std::min(n_out, chz_t_max(z));
    const uint64_t n_wgs = (uint64_t)z->n_src * ((n_out + t_blk - 1) / t_blk) * ((z->sv_tiles.size() + CHZ_WAVES - 1) / CHZ_WAVES);
    if (n_res > 0x3fffffffull || n_wgs > 0x7fffffffull) return z->fail(IQD_EINVAL, "channelizer: survey too large for one call");
    return IQD_OK;
}

int iqd_channelizer_survey_device(iqd_channelizer_t *z, const void *wide_dev, size_t bytes_per_source, uint32_t block_bytes,
                                  void *magnitude_dev)
{
    if (!z) return IQD_EINVAL;
    if (!wide_dev || !magnitude_dev) return z->fail(IQD_EINVAL, "channelizer: NULL buffer");
    if ((((uintptr_t)wide_dev) | ((uintptr_t)magnitude_dev)) & 15) return z->fail(IQD_EINVAL, "channelizer: buffers must be 16-byte aligned");
    int rc = chz_survey_check(z, bytes_per_source, block_bytes);
    if (rc != IQD_OK) return rc;
    (void)hipSetDevice(z->device);
    if (z->sv_dirty) {
        rc = chz_survey_upload(z);
        if (rc != IQD_OK) return rc;
    }
    ChzLaunch a = chz_launch(z, wide_dev, bytes_per_source);   // (the history read only: a survey looks and does not touch)
    a.amat = z->d_sv_amat.as<uint4>();
    a.tiles = z->d_sv_tiles.as<ChzTile>();
    const uint32_t n_out = a.n_out;
    ChzSurveyLaunch s{};
    s.sums = (uint32_t *)magnitude_dev;
    s.n_points = (uint32_t)z->sv_inc.size();
    s.n_tiles = (uint32_t)z->sv_tiles.size();
    s.block_out = block_bytes / 2;
    s.n_blocks = n_out / s.block_out;
    s.n_win = (n_out + a.t_blk - 1) / a.t_blk;
    s.rows = (s.n_tiles + CHZ_WAVES - 1) / CHZ_WAVES;
    CHZ_TRY(z, hipMemsetAsync(magnitude_dev, 0, (size_t)z->n_src * s.n_blocks * s.n_points * 4, z->stream));
    CHZ_TRY(z, launch_channelizer_survey(a, s, z->stream));
    return IQD_OK;
}

int iqd_channelizer_survey(iqd_channelizer_t *z, const uint8_t *wide, size_t bytes_per_source, uint32_t block_bytes, uint32_t *magnitude)
{
    if (!z) return IQD_EINVAL;
    if (!wide || !magnitude) return z->fail(IQD_EINVAL, "channelizer: NULL buffer");
    int rc = chz_survey_check(z, bytes_per_source, block_bytes);
    if (rc != IQD_OK) return rc;
    (void)hipSetDevice(z->device);
    const size_t ib = (size_t)z->n_src * bytes_per_source;
    const size_t ob = (size_t)z->n_src * (bytes_per_source / z->m * z->q / block_bytes) * z->sv_inc.size() * 4;
    CHZ_TRY(z, z->st_wide.ensure(ib));
    CHZ_TRY(z, z->sv_mag.ensure(ob));
    CHZ_TRY(z, hipMemcpyAsync(z->st_wide.p, wide, ib, hipMemcpyHostToDevice, z->stream));
    rc = iqd_channelizer_survey_device(z, z->st_wide.p, bytes_per_source, block_bytes, z->sv_mag.p);
    if (rc != IQD_OK) return rc;
    CHZ_TRY(z, hipMemcpyAsync(magnitude, z->sv_mag.p, ob, hipMemcpyDeviceToHost, z->stream));
    CHZ_TRY(z, hipStreamSynchronize(z->stream));
    return IQD_OK;
}

// DbfsCalculator's table as the squelch reads it (build_consts' db_table, magnitude_dbfs in iqd_chains.h)
int32_t iqd_magnitude_dbfs(uint32_t magnitude)
{
    static const std::vector<int32_t> table = [] {
        Consts c;
        build_consts(c);
        return std::vector<int32_t>(c.db_table, c.db_table + 128);
    }();
    return table[magnitude > 127u ? 127u : magnitude] - 42;
}

// Checks and queues one wideband accept: the rows into rows_dev, then iqd_accept_iq_device on them.  With following
// channels the engine's pending settings are applied first (once), so that the walker reads the state the accept starts
// from.
static int wideband_queue(iqd_t *e, iqd_channelizer *z, uint32_t first_ch, const void *wide_dev, size_t bytes_per_source,
                          void *rows_dev, void *pcm_dev, void *pcm_count_dev, void *magnitude_dev, void *signal_present_dev)
{
    if (!z || z->e != e) return engine_fail(e, IQD_EINVAL, "accept_wideband: the channelizer belongs to another engine");
    if (!wide_dev || !rows_dev || !pcm_dev) return z->fail(IQD_EINVAL, "accept_wideband: NULL buffer");
    if ((((uintptr_t)wide_dev) | ((uintptr_t)rows_dev)) & 15) return z->fail(IQD_EINVAL, "accept_wideband: wide and rows buffers must be 16-byte aligned");
    int rc = chz_check_len(z, bytes_per_source);
    if (rc == IQD_OK) rc = chz_check_tracks(z, bytes_per_source);
    if (rc != IQD_OK) return rc;
    uint32_t e_nch = 0, bb = 0, flags = 0;
    engine_geometry(e, &e_nch, &bb, &flags);
    if (first_ch >= e_nch || z->n_ch > e_nch - first_ch) return z->fail(IQD_EINVAL, "accept_wideband: bad engine channel range");
    const size_t row = z->row_bytes(bytes_per_source);
    if (row % bb != 0 && (row >= bb || row % 64 != 0))
        return z->fail(IQD_EINVAL, "accept_wideband: bytes_per_source / decimation must be a multiple of block_bytes, or one short block");
    const size_t nblk = row % bb == 0 ? row / bb : 1;
    (void)hipSetDevice(z->device);
    if (z->n_follow || z->n_gain) {
        ChzScanLaunch sl{};
        rc = engine_settle(e, &sl);
        if (rc != IQD_OK) return rc;
        sl.first_ch = first_ch;
        sl.n_blocks = (uint32_t)nblk;
        sl.block_out = (uint32_t)(row / nblk / 2);
        rc = chz_queue(z, wide_dev, bytes_per_source, rows_dev, &sl);
    } else {
        rc = chz_queue(z, wide_dev, bytes_per_source, rows_dev, nullptr);
    }
    if (rc != IQD_OK) return rc;
    if (flags & IQD_F_PREPASS_OVERLAP) CHZ_TRY(z, hipStreamSynchronize(z->stream));   // that path wants its input complete
    rc = iqd_accept_iq_device(e, first_ch, z->n_ch, rows_dev, row, pcm_dev, pcm_count_dev, magnitude_dev, signal_present_dev);
    if (rc != IQD_OK) {
        // The checks above are the engine's own (range, block_bytes rule), so it does not refuse these rows; should it
        // still, the channelizer steps back as well: the call's history went to the other buffer, so the stream stands
        // where it stood before the call, like the engine's.
        z->cur ^= 1;
        if (z->track_ran) z->carry_cur ^= 1;
        z->m_abs -= z->row_bytes(bytes_per_source) / 2;
        return rc;
    }
    return IQD_OK;
}

int iqd_accept_wideband(iqd_t *e, iqd_channelizer_t *z, uint32_t first_ch, const uint8_t *wide, size_t bytes_per_source,
                        int16_t *pcm, uint32_t *pcm_count, uint32_t *magnitude, uint8_t *signal_present)
{
    if (!e) return IQD_EINVAL;
    if (!z || z->e != e) return engine_fail(e, IQD_EINVAL, "accept_wideband: the channelizer belongs to another engine");
    if (!wide || !pcm) return z->fail(IQD_EINVAL, "accept_wideband: NULL buffer");
    int rc = chz_check_len(z, bytes_per_source);
    if (rc == IQD_OK) rc = chz_check_tracks(z, bytes_per_source);
    if (rc != IQD_OK) return rc;
    uint32_t e_nch = 0, bb = 0, flags = 0;
    engine_geometry(e, &e_nch, &bb, &flags);
    const size_t row = z->row_bytes(bytes_per_source);
    const size_t nblk = row % bb == 0 ? row / bb : 1;
    (void)hipSetDevice(z->device);
    const size_t n = z->n_ch, ib = (size_t)z->n_src * bytes_per_source;
    CHZ_TRY(z, z->st_wide.ensure(ib));
    CHZ_TRY(z, z->w_rows.ensure(n * row));
    CHZ_TRY(z, z->w_pcm.ensure(n * (row / 64) * 2));
    CHZ_TRY(z, z->w_cnt.ensure(n * 4));
    CHZ_TRY(z, z->w_mag.ensure(n * nblk * 4));
    CHZ_TRY(z, z->w_sp.ensure(n * nblk));
    CHZ_TRY(z, hipMemcpyAsync(z->st_wide.p, wide, ib, hipMemcpyHostToDevice, z->stream));
    rc = wideband_queue(e, z, first_ch, z->st_wide.p, bytes_per_source, z->w_rows.p, z->w_pcm.p, z->w_cnt.p,
                        magnitude ? z->w_mag.p : nullptr, signal_present ? z->w_sp.p : nullptr);
    if (rc != IQD_OK) return rc;
    CHZ_TRY(z, hipMemcpyAsync(pcm, z->w_pcm.p, n * (row / 64) * 2, hipMemcpyDeviceToHost, z->stream));
    if (pcm_count) CHZ_TRY(z, hipMemcpyAsync(pcm_count, z->w_cnt.p, n * 4, hipMemcpyDeviceToHost, z->stream));
    if (magnitude) CHZ_TRY(z, hipMemcpyAsync(magnitude, z->w_mag.p, n * nblk * 4, hipMemcpyDeviceToHost, z->stream));
    if (signal_present) CHZ_TRY(z, hipMemcpyAsync(signal_present, z->w_sp.p, n * nblk, hipMemcpyDeviceToHost, z->stream));
    CHZ_TRY(z, hipStreamSynchronize(z->stream));
    return IQD_OK;
}

int iqd_accept_wideband_device(iqd_t *e, iqd_channelizer_t *z, uint32_t first_ch, const void *wide_dev, size_t bytes_per_source,
                               void *rows_dev, void *pcm_dev, void *pcm_count_dev, void *magnitude_dev, void *signal_present_dev)
{
    if (!e) return IQD_EINVAL;
    return wideband_queue(e, z, first_ch, wide_dev, bytes_per_source, rows_dev, pcm_dev, pcm_count_dev, magnitude_dev,
                          signal_present_dev);
}

int iqd_channelizer_set_source_frequency(iqd_channelizer_t *z, uint32_t first_source, uint32_t n, const uint64_t *centre_hz)
{
    if (!z) return IQD_EINVAL;
    if (!centre_hz || n < 1 || first_source >= z->n_src || n > z->n_src - first_source)
        return z->fail(IQD_EINVAL, "channelizer: bad source range");
    for (uint32_t i = 0; i < n; i++) z->centre[first_source + i] = centre_hz[i];
    z->centre_dirty = true;
    return IQD_OK;
}

// One kind of following for channels [first, first + n): flags / count are that kind's, other the other kind's flags;
// msg: S16 captures, S8 captures, a fractional channelizer, a channel of the other kind
static int chz_follow(iqd_channelizer *z, uint32_t first, uint32_t n, int follow, std::vector<uint8_t> &flags,
                      const std::vector<uint8_t> &other, uint32_t &count, const char *const (&msg)[4])
{
    if (n < 1 || first >= z->n_ch || n > z->n_ch - first) return z->fail(IQD_EINVAL, "channelizer: bad channel range");
    if (follow && z->fmt != IQD_WIDE_U8) return z->fail(IQD_EINVAL, msg[z->fmt == IQD_WIDE_S16 ? 0 : 1]);
    if (follow && z->q > 1) return z->fail(IQD_EINVAL, msg[2]);
    for (uint32_t i = 0; follow && i < n; i++) {
        if (other[first + i]) return z->fail(IQD_EINVAL, msg[3]);
        if (z->trk[first + i] >= 0)
            return z->fail(IQD_EINVAL, "channelizer: a channel that follows a track slot cannot follow its scanner or its gain as well (not built yet)");
    }
    for (uint32_t i = 0; i < n; i++) {
        uint8_t &f = flags[first + i];
        if (f == (follow ? 1 : 0)) continue;
        f = follow ? 1 : 0;
        count += follow ? 1 : -1;
        z->layout_dirty = true;
    }
    return IQD_OK;
}

int iqd_channelizer_follow_scanner(iqd_channelizer_t *z, uint32_t first, uint32_t n, int follow)
{
    static const char *const msg[4] = {
        "channelizer: channels on IQD_WIDE_S16 captures cannot follow a scanner yet",
        "channelizer: channels on IQD_WIDE_S8 captures cannot follow a scanner yet",
        "channelizer: channels of a fractional channelizer (decimation_den > 1) cannot follow a scanner",
        "channelizer: a channel that follows its gain cannot follow its scanner as well (not built yet)"};
    return z ? chz_follow(z, first, n, follow, z->follow, z->follow_gain, z->n_follow, msg) : IQD_EINVAL;
}

int iqd_channelizer_follow_gain(iqd_channelizer_t *z, uint32_t first, uint32_t n, int follow)
{
    static const char *const msg[4] = {
        "channelizer: channels on IQD_WIDE_S16 captures cannot follow their gain yet",
        "channelizer: channels on IQD_WIDE_S8 captures cannot follow their gain yet",
        "channelizer: channels of a fractional channelizer (decimation_den > 1) cannot follow their gain yet",
        "channelizer: a channel that follows its scanner cannot follow its gain as well (not built yet)"};
    return z ? chz_follow(z, first, n, follow, z->follow_gain, z->follow, z->n_gain, msg) : IQD_EINVAL;
}

int iqd_channelizer_set_track_table(iqd_channelizer_t *z, const iqd_track_follow *t)
{
    if (!z) return IQD_EINVAL;
    if (!t) {
        z->table = iqd_track_follow{};
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
    z->table = *t;
    return IQD_OK;
}

int iqd_channelizer_follow_tracks(iqd_channelizer_t *z, uint32_t first, uint32_t n, const int32_t *slot)
{
    if (!z) return IQD_EINVAL;
    if (n < 1 || first >= z->n_ch || n > z->n_ch - first) return z->fail(IQD_EINVAL, "channelizer: bad channel range");
    for (uint32_t i = 0; slot && i < n; i++) {
        if (slot[i] < -1 || slot[i] > 63) return z->fail(IQD_EINVAL, "channelizer: a track slot must be -1 or 0..63");
        if (slot[i] < 0) continue;
        if (z->fmt != IQD_WIDE_U8)
            return z->fail(IQD_EINVAL, z->fmt == IQD_WIDE_S16 ? "channelizer: channels on IQD_WIDE_S16 captures cannot follow tracks yet"
                                                              : "channelizer: channels on IQD_WIDE_S8 captures cannot follow tracks yet");
        if (z->q > 1) return z->fail(IQD_EINVAL, "channelizer: channels of a fractional channelizer (decimation_den > 1) cannot follow tracks yet");
        if (z->follow[first + i]) return z->fail(IQD_EINVAL, "channelizer: a channel that follows its scanner cannot follow a track slot as well (not built yet)");
        if (z->follow_gain[first + i]) return z->fail(IQD_EINVAL, "channelizer: a channel that follows its gain cannot follow a track slot as well (not built yet)");
    }
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t c = first + i;
        const int32_t s = slot ? slot[i] : -1;
        if (s == z->trk[c]) continue;
        if ((s >= 0) != (z->trk[c] >= 0)) {
            z->n_track += s >= 0 ? 1 : -1;
            z->layout_dirty = true;
        }
        z->trk[c] = s;
        z->trk_fresh[c] = s >= 0;   // a channel that starts to follow, or moves to another slot: its carry does not count
        z->any_fresh = z->any_fresh || s >= 0;
        z->ch_dirty[c] = 1;
        z->any_dirty = true;
    }
    return IQD_OK;
}

// chz_track_window_outputs as a host-only function
uint32_t iqd_channelizer_track_window_outputs(uint32_t decimation, uint32_t n_taps)
{
    if (decimation < 2 || decimation > 64 || n_taps < 1 || n_taps > 1024) return 0;
    return chz_track_window_outputs(decimation, (n_taps + 31) / 32 * 32);
}

// chz_t_max as a host-only function (the window's fit in LDS is checked on it for every M)
uint32_t iqd_channelizer_window_outputs(uint32_t decimation, uint32_t n_taps, uint32_t sample_format)
{
    if (decimation < 2 || decimation > 64 || n_taps < 1 || n_taps > 1024 || sample_format > IQD_WIDE_S16) return 0;
    return chz_window_outputs(decimation, (n_taps + 31) / 32 * 32, 1, sample_format == IQD_WIDE_S16 ? 2 : 1);
}

int iqd_channelizer_tuning(uint32_t decimation, uint64_t source_centre_hz, uint64_t station_hz, int rotation, uint32_t *inc)
{
    if (decimation < 2 || decimation > 64 || rotation < -1 || rotation > 1 || !inc) return IQD_EINVAL;
    return chz_tuning(decimation, source_centre_hz, station_hz, rotation, inc) ? IQD_OK : IQD_EINVAL;
}

}  // extern "C"
