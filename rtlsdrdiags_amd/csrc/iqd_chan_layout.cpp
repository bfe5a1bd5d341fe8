// Wideband channelizer, host side: channels -> taps -> tiles -> A operands -> upload pieces (iqd_chan_layout.h).  No HIP call.
#include "iqd_chan_layout.h"

#include <algorithm>

namespace iqd {

ChzGeometry::ChzGeometry(const iqd_channelizer_config &cfg, std::vector<int16_t> taps)
    : n_src(cfg.n_sources), n_ch(cfg.n_channels), m(cfg.decimation), k((uint32_t)taps.size()),
      q(cfg.decimation_den ? cfg.decimation_den : 1), fmt(cfg.sample_format), rail(cfg.sample_format == IQD_WIDE_S16 ? 2 : 1),
      h(std::move(taps)), phasor(2 * CHZ_PHASOR)
{
    kb = (k + q - 1) / q;
    kp = (kb + 31) / 32 * 32;
    nq = kp / 32;
    chz_phasor_table(phasor.data());
}

void chz_channel_taps(const int16_t *h, uint32_t k, uint32_t inc, const int16_t *phasor, int16_t *gr, int16_t *gi)
{
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t i = (uint32_t)(j * inc) >> 20;
        gr[j] = (int16_t)(((int32_t)h[j] * phasor[2 * i] + (1 << 14)) >> 15);
        gi[j] = (int16_t)(((int32_t)h[j] * phasor[2 * i + 1] + (1 << 14)) >> 15);
    }
}

// branch r of the prototype is h_r[k] = h[k q + r], k < ceil((K - r) / q) (q = 1: the prototype itself)
void chz_branch_taps(const ChzGeometry &g, uint32_t inc, int16_t *gr, int16_t *gi)
{
    std::vector<int16_t> hr(g.kb);
    for (uint32_t r = 0; r < g.q; r++) {
        const uint32_t kr = g.k > r ? (g.k - r + g.q - 1) / g.q : 0;
        for (uint32_t k = 0; k < kr; k++) hr[k] = g.h[(size_t)k * g.q + r];
        chz_channel_taps(hr.data(), kr, inc, g.phasor.data(), gr + (size_t)r * g.kb, gi + (size_t)r * g.kb);
    }
}

void ChzChannels::create(const ChzGeometry &g)
{
    src.assign(g.n_ch, 0);
    inc.assign(g.n_ch, 0);
    shift.assign(g.n_ch, 0);
    kind.assign(g.n_ch, CHZ_FIXED);
    n_kind[CHZ_FIXED] = g.n_ch;
    trk.assign(g.n_ch, -1);
    trk_fresh.assign(g.n_ch, 0);
    gr.assign(g.n_ch * g.taps_per_channel(), 0);
    gi.assign(g.n_ch * g.taps_per_channel(), 0);
    ch_dirty.assign(g.n_ch, 0);
    for (uint32_t c = 0; c < g.n_ch; c++) new_taps(g, c);
}

void ChzChannels::new_taps(const ChzGeometry &g, uint32_t c)
{
    const size_t at = c * g.taps_per_channel();
    chz_branch_taps(g, inc[c], &gr[at], &gi[at]);
    ch_dirty[c] = 1;
    any_dirty = true;
}

void ChzChannels::set_kind(uint32_t c, int k)
{
    if (kind[c] == k) return;
    n_kind[kind[c]]--;
    n_kind[k]++;
    kind[c] = (uint8_t)k;
    layout_dirty = true;
}

void ChzChannels::clean()
{
    std::fill(ch_dirty.begin(), ch_dirty.end(), 0);
    layout_dirty = false;
    any_dirty = false;
}

ChzSpan ChzLayout::array(int a) const
{
    if (a == CHZ_AMAT) return {amat.data(), amat.size()};
    if (a == CHZ_TILES) return {tiles.data(), tiles.size() * sizeof(ChzTile)};
    if (a == CHZ_GSUM) return {gsum.data(), gsum.size() * sizeof(ChzFmtTile)};
    return {wg[a - CHZ_WGS].wgs.data(), wg[a - CHZ_WGS].wgs.size() * sizeof(ChzWg)};
}

// A walker's workgroups take `waves` tiles each: as few as keep every CU busy; the rest of the workgroup's 8 waves share the
// tiles' outputs (wpt waves per tile).
static void chz_walker_wgs(const ChzGeometry &g, const std::vector<ChzWg> &runs, ChzWgSet &w)
{
    uint32_t n_tiles = 0;
    for (const ChzWg &r : runs) n_tiles += r.n_tiles;
    w.waves = std::max(1u, std::min(CHZ_WAVES, n_tiles / std::max(1u, g.n_cus)));
    w.wpt = 1;
    while (2 * w.wpt * w.waves <= CHZ_WAVES) w.wpt *= 2;
    for (const ChzWg &r : runs)
        for (uint32_t t = 0; t < r.n_tiles; t += w.waves)
            w.wgs.push_back(ChzWg{r.source, r.first_tile + t, std::min(w.waves, r.n_tiles - t), 0});
}

// channels sorted by kind, then by source, 8 per tile, up to CHZ_WAVES tiles of one source per workgroup row; channels of
// different kinds never share a tile.
void ChzLayout::group(const ChzGeometry &g, const ChzChannels &ch)
{
    tiles.clear();
    for (ChzWgSet &w : wg) w.wgs.clear();
    slot_of.assign(g.n_ch, 0);
    std::vector<std::vector<uint32_t>> by_src[CHZ_KINDS];
    for (auto &b : by_src) b.resize(g.n_src);
    for (uint32_t c = 0; c < g.n_ch; c++) by_src[ch.kind[c]][ch.src[c]].push_back(c);
    std::vector<ChzWg> runs[CHZ_KINDS];           // following tiles per source
    for (int f = 0; f < CHZ_KINDS; f++) {
        first_tile[f] = (uint32_t)tiles.size();
        for (uint32_t s = 0; s < g.n_src; s++) {
            const auto &list = by_src[f][s];
            const uint32_t first = (uint32_t)tiles.size();
            for (size_t i = 0; i < list.size(); i += CHZ_TILE_CH) {
                ChzTile t;
                for (uint32_t l = 0; l < CHZ_TILE_CH; l++) {
                    t.ch[l] = i + l < list.size() ? list[i + l] : CHZ_NONE;
                    if (t.ch[l] != CHZ_NONE) slot_of[t.ch[l]] = (uint32_t)tiles.size() * CHZ_TILE_CH + l;
                }
                tiles.push_back(t);
            }
            const uint32_t n_tiles = (uint32_t)tiles.size() - first;
            if (f == CHZ_FIXED || f == CHZ_TRACK)   // chz_kernel's geometry: rows of up to CHZ_WAVES tiles
                for (uint32_t t = 0; t < n_tiles; t += CHZ_WAVES)
                    wg[f].wgs.push_back(ChzWg{s, first + t, std::min(CHZ_WAVES, n_tiles - t), 0});
            else if (n_tiles)
                runs[f].push_back(ChzWg{s, first, n_tiles, 0});
        }
    }
    first_tile[CHZ_KINDS] = (uint32_t)tiles.size();
    chz_walker_wgs(g, runs[CHZ_GAIN], wg[CHZ_GAIN]);
    chz_walker_wgs(g, runs[CHZ_SCAN], wg[CHZ_SCAN]);
    amat.assign(tiles.size() * g.tile_bytes(), 0);
    if (g.fmt == IQD_WIDE_S16) gsum.assign(tiles.size(), ChzFmtTile{});
}

// A operands of one tile slot (iqd_chan.h) into amat: rows 2 l (Ar) and 2 l + 1 (Ai), both planes, every K-chunk, for
// every output residue res (its branch: ((res + 1) m - 1) mod q).  gr / gi [q][kb]: the slot's taps, NULL = padding (zeros)
static void chz_pack_rows(const ChzGeometry &g, uint8_t *amat, uint32_t tile, uint32_t l, const int16_t *gr, const int16_t *gi)
{
    for (uint32_t res = 0; res < g.q; res++) {
        const uint32_t br = (uint32_t)((((uint64_t)res + 1) * g.m - 1) % g.q);
        const size_t taps = (size_t)br * g.kb;
        for (uint32_t row = 0; row < 2; row++) {
            const uint32_t rho = 2 * l + row;
            for (uint32_t q = 0; q < g.nq; q++)
                for (uint32_t grp = 0; grp < 4; grp++)
                    for (uint32_t j = 0; j < 16; j++) {
                        const uint32_t kappa = 64 * q + 16 * grp + j, comp = kappa & 1;
                        const uint32_t kk = g.kp - 1 - kappa / 2;
                        int32_t v = 0;
                        if (gr && kk < g.kb) {
                            const int32_t r = gr[taps + kk], i = gi[taps + kk];
                            v = row == 0 ? (comp == 0 ? r : -i) : (comp == 0 ? i : r);
                        }
                        const int8_t lo = (int8_t)(v & 0xff);
                        const int8_t hi = (int8_t)((v - lo) / 256);
                        const size_t lane = rho + 16 * grp;
                        for (uint32_t p = 0; p < 2; p++)
                            amat[(((((size_t)tile * g.q + res) * g.nq + q) * 2 + p) * 64 + lane) * 16 + j] =
                                (uint8_t)(p == 0 ? lo : hi);
                    }
        }
    }
}

void chz_pack_slot(const ChzGeometry &g, ChzTile &t, uint32_t tile, uint32_t l, uint32_t ch, uint32_t inc, uint32_t shift,
                   const int16_t *gr, const int16_t *gi, uint8_t *amat, ChzFmtTile *gsum)
{
    const bool pad = ch == CHZ_NONE;
    t.ch[l] = ch;
    t.inc[l] = pad ? 0 : inc;
    t.shift[l] = pad ? 0 : shift;
    if (!amat) return;
    chz_pack_rows(g, amat, tile, l, pad ? nullptr : gr, pad ? nullptr : gi);
    if (gsum) {   // the sums of rows 2 l (gr on I, -gi on Q) and 2 l + 1 (gi on I, gr on Q); |sum| < 2^25
        int32_t sr = 0, si = 0;
        for (uint32_t k = 0; !pad && k < g.kb; k++) {
            sr += gr[k];
            si += gi[k];
        }
        gsum[tile].g[l][0] = sr - si;
        gsum[tile].g[l][1] = sr + si;
    }
}

std::vector<ChzPiece> ChzLayout::repack(const ChzGeometry &g, const ChzChannels &ch, bool *regrouped)
{
    const bool regroup = *regrouped = ch.layout_dirty;
    if (regroup) group(g, ch);
    const size_t n_tiles = tiles.size(), n_packed = first_tile[CHZ_SCAN], tile_bytes = g.tile_bytes();
    std::vector<uint8_t> tile_dirty(n_tiles, regroup ? 1 : 0);
    for (uint32_t t = 0; t < n_tiles; t++)
        for (uint32_t l = 0; l < CHZ_TILE_CH; l++) {
            const uint32_t c = tiles[t].ch[l];
            if (!regroup && (c == CHZ_NONE || !ch.ch_dirty[c])) continue;
            uint8_t *const a = t < n_packed ? amat.data() : nullptr;
            ChzFmtTile *const sums = g.fmt == IQD_WIDE_S16 ? gsum.data() : nullptr;
            tile_dirty[t] = 1;
            if (c == CHZ_NONE) {                  // padding: zeros
                chz_pack_slot(g, tiles[t], t, l, CHZ_NONE, 0, 0, nullptr, nullptr, a, sums);
                continue;
            }
            // a track follower: the slot it follows in the increment's place (iqd_chan.h)
            const uint32_t inc = t >= first_tile[CHZ_TRACK] ? (uint32_t)ch.trk[c] | (ch.trk_fresh[c] ? CHZ_TRACK_FRESH : 0u) : ch.inc[c];
            const size_t taps = c * g.taps_per_channel();
            chz_pack_slot(g, tiles[t], t, l, c, inc, ch.shift[c], &ch.gr[taps], &ch.gi[taps], a, sums);
        }
    std::vector<ChzPiece> pieces;
    for (size_t t = 0; t < n_tiles; t++) {
        if (!tile_dirty[t]) continue;
        size_t n = 1;                             // a run of consecutive dirty tiles
        while (t + n < n_tiles && tile_dirty[t + n]) n++;
        const size_t na = t < n_packed ? std::min(n, n_packed - t) : 0;
        if (na) pieces.push_back({CHZ_AMAT, t * tile_bytes, na * tile_bytes});
        pieces.push_back({CHZ_TILES, t * sizeof(ChzTile), n * sizeof(ChzTile)});
        if (g.fmt == IQD_WIDE_S16) pieces.push_back({CHZ_GSUM, t * sizeof(ChzFmtTile), n * sizeof(ChzFmtTile)});
        t += n;                                   // (tile t + n is clean, or the end)
    }
    for (int k = 0; k < CHZ_KINDS; k++)
        if (regroup && !wg[k].wgs.empty()) pieces.push_back({CHZ_WGS + k, 0, array(CHZ_WGS + k).bytes});
    return pieces;
}

}  // namespace iqd
