// tests/chan_layout — TEST INFRASTRUCTURE ONLY: the channelizer's layout code (rtlsdrdiags_amd/csrc/iqd_chan_layout.cpp, with
// iqd_chan_design.cpp for the phasor table) on the host.  No HIP call is made and no HIP library is linked;
// tests/test_chan_layout.py builds this with AddressSanitizer + UBSan, so an index outside an array fails the run too.
//   packing:  every A-operand byte unpacks to the tap it came from (lo + 256 hi at the kappa -> (k, rail) position that
//             iqd_chan.h states), padding is zero, the S16 row sums are the rows' sums
//   grouping: every channel in exactly one slot, one source and one kind per tile, kinds in order, every tile of a kind in
//             exactly one workgroup row of that kind
//   pieces:   after a retune exactly the dirty tiles, inside the arrays (U8, and S16 with its row sums); after a source change
//             everything; the same again until the caller says they were queued (ChzChannels::clean)
#include <stdio.h>

#include <set>
#include <vector>

#include "iqd_chan_layout.h"

using namespace iqd;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static uint32_t rng_state = 12345;
static uint32_t rnd()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static ChzGeometry geometry(uint32_t n_src, uint32_t n_ch, uint32_t m, uint32_t q, uint32_t k, uint32_t fmt)
{
    iqd_channelizer_config cfg{};
    cfg.n_sources = n_src;
    cfg.n_channels = n_ch;
    cfg.decimation = m;
    cfg.decimation_den = q;
    cfg.sample_format = fmt;
    std::vector<int16_t> h(k);
    for (int16_t &t : h) t = (int16_t)((int)(rnd() % 65279) - 32639);
    h[0] = 32639;
    h[k - 1] = -32639;
    return ChzGeometry(cfg, h);
}

// ---- packing ------------------------------------------------------------------------------------------------------------------

static void check_packing(uint32_t q, uint32_t k, bool sums)
{
    const uint32_t m = q == 1 ? 8 : q == 8 ? 75 : 9, n_ch = 11;
    const ChzGeometry g = geometry(2, n_ch, m, q, k, sums ? IQD_WIDE_S16 : IQD_WIDE_U8);
    CHECK(g.kb == (k + q - 1) / q && g.kp % 32 == 0 && g.kp >= g.kb && g.kp < g.kb + 32 && g.nq == g.kp / 32);
    ChzChannels ch;
    ch.create(g);
    for (uint32_t c = 0; c < n_ch; c++) {
        ch.src[c] = c % 2;
        ch.inc[c] = c == 0 ? 0 : c == 1 ? 0x80000000u : rnd() << 8 | (rnd() & 0xff);
        ch.shift[c] = c % 9;
        ch.new_taps(g, c);
    }
    ChzLayout lay;
    bool regrouped = false;
    lay.repack(g, ch, &regrouped);
    CHECK(regrouped && lay.tiles.size() == 2 && lay.amat.size() == 2 * g.tile_bytes());   // 6 and 5 channels: padding in both
    // the taps: branch r of the prototype, rotated by the phasor at (k inc) >> 20, k the index within the branch
    for (uint32_t c = 0; c < n_ch; c++)
        for (uint32_t r = 0; r < q; r++)
            for (uint32_t i = 0; i < g.kb; i++) {
                const size_t at = c * g.taps_per_channel() + (size_t)r * g.kb + i, src = (size_t)i * q + r;
                const uint32_t ph = (uint32_t)(i * ch.inc[c]) >> 20;
                const int32_t hh = src < k ? g.h[src] : 0;
                CHECK(ch.gr[at] == (int16_t)((hh * g.phasor[2 * ph] + (1 << 14)) >> 15));
                CHECK(ch.gi[at] == (int16_t)((hh * g.phasor[2 * ph + 1] + (1 << 14)) >> 15));
            }
    size_t at = 0;
    for (uint32_t tile = 0; tile < lay.tiles.size(); tile++)
        for (uint32_t res = 0; res < q; res++) {
            const uint32_t br = (uint32_t)((((uint64_t)res + 1) * m - 1) % q);
            for (uint32_t qc = 0; qc < g.nq; qc++)
                for (uint32_t lane = 0; lane < 64; lane++)
                    for (uint32_t j = 0; j < 16; j++) {
                        const size_t lo_at = ((((size_t)tile * q + res) * g.nq + qc) * 2 * 64 + lane) * 16 + j, hi_at = lo_at + 64 * 16;
                        const uint32_t rho = lane % 16, grp = lane / 16, l = rho / 2, row = rho % 2;
                        const uint32_t kappa = 64 * qc + 16 * grp + j, kk = g.kp - 1 - kappa / 2, rail = kappa & 1;
                        const uint32_t c = lay.tiles[tile].ch[l];
                        int32_t want = 0;
                        if (c != CHZ_NONE && kk < g.kb) {
                            const size_t tap = c * g.taps_per_channel() + (size_t)br * g.kb + kk;
                            want = row == 0 ? (rail == 0 ? ch.gr[tap] : -ch.gi[tap]) : (rail == 0 ? ch.gi[tap] : ch.gr[tap]);
                        }
                        CHECK((int8_t)lay.amat[lo_at] + 256 * (int8_t)lay.amat[hi_at] == want);
                        at += 2;
                    }
        }
    CHECK(at == lay.amat.size());                   // every byte was looked at
    for (uint32_t tile = 0; tile < lay.tiles.size(); tile++)
        for (uint32_t l = 0; l < CHZ_TILE_CH; l++) {
            const uint32_t c = lay.tiles[tile].ch[l];
            CHECK(lay.tiles[tile].inc[l] == (c == CHZ_NONE ? 0 : ch.inc[c]) && lay.tiles[tile].shift[l] == (c == CHZ_NONE ? 0u : ch.shift[c]));
            if (!sums) continue;
            int32_t sr = 0, si = 0;
            for (uint32_t i = 0; c != CHZ_NONE && i < g.kb; i++) {
                sr += ch.gr[c * g.taps_per_channel() + i];
                si += ch.gi[c * g.taps_per_channel() + i];
            }
            CHECK(lay.gsum[tile].g[l][0] == sr - si && lay.gsum[tile].g[l][1] == sr + si);
        }
    CHECK(sums ? lay.gsum.size() == lay.tiles.size() : lay.gsum.empty());
}

// ---- grouping -----------------------------------------------------------------------------------------------------------------

// channels of every kind on n_src sources, (kind, source) pairs taking 1, 8, 9, 65 and 0 channels in turn, handed out in a
// shuffled order; ch is created and set up on g
static void mixed_channels(ChzGeometry &g, ChzChannels &ch, uint32_t n_src, uint32_t n_cus, uint32_t fmt = IQD_WIDE_U8)
{
    static const uint32_t COUNTS[5] = {1, 8, 9, 65, 0};
    std::vector<uint32_t> kind, src;
    uint32_t turn = n_src;
    for (int k = 0; k < CHZ_KINDS; k++)
        for (uint32_t s = 0; s < n_src; s++, turn++)
            for (uint32_t i = 0; i < COUNTS[turn % 5]; i++) {
                kind.push_back(fmt == IQD_WIDE_U8 ? (uint32_t)k : (uint32_t)CHZ_FIXED);
                src.push_back(s);
            }
    g = geometry(n_src, (uint32_t)kind.size(), 8, 1, 33, fmt);
    g.n_cus = n_cus;
    ch = ChzChannels();
    ch.create(g);
    for (uint32_t c = g.n_ch; c > 1; c--) {
        const uint32_t o = rnd() % c;
        std::swap(kind[c - 1], kind[o]);
        std::swap(src[c - 1], src[o]);
    }
    for (uint32_t c = 0; c < g.n_ch; c++) {
        ch.src[c] = src[c];
        ch.inc[c] = rnd() << 8;
        ch.set_kind(c, (int)kind[c]);
        if (kind[c] == CHZ_TRACK) {
            ch.trk[c] = (int32_t)(c % 64);
            ch.trk_fresh[c] = c % 2;
        }
        ch.new_taps(g, c);
    }
}

static void check_grouping(uint32_t n_src, uint32_t n_cus)
{
    ChzGeometry g;
    ChzChannels ch;
    mixed_channels(g, ch, n_src, n_cus);
    uint32_t total = 0;
    for (int k = 0; k < CHZ_KINDS; k++) total += ch.n_kind[k];
    CHECK(total == g.n_ch);
    ChzLayout lay;
    bool regrouped = false;
    lay.repack(g, ch, &regrouped);
    const uint32_t n_tiles = (uint32_t)lay.tiles.size();
    CHECK(regrouped && lay.first_tile[0] == 0 && lay.first_tile[CHZ_KINDS] == n_tiles && lay.slot_of.size() == g.n_ch);
    std::vector<uint32_t> seen(g.n_ch, 0);
    int last_source = -1, last_kind = -1;
    for (int k = 0; k < CHZ_KINDS; k++) {
        CHECK(lay.first_tile[k] <= lay.first_tile[k + 1]);
        uint32_t n_of_kind = 0;
        std::vector<uint32_t> covered(n_tiles, 0);
        for (uint32_t t = lay.first_tile[k]; t < lay.first_tile[k + 1] && t < n_tiles; t++) {
            const ChzTile &T = lay.tiles[t];
            CHECK(T.ch[0] != CHZ_NONE);             // no empty tile, and the padding comes last
            const uint32_t source = T.ch[0] != CHZ_NONE ? ch.src[T.ch[0]] : 0;
            CHECK(last_kind != k || (int)source >= last_source);   // a kind's tiles: sources in order
            last_kind = k;
            last_source = (int)source;
            for (uint32_t l = 0; l < CHZ_TILE_CH; l++) {
                const uint32_t c = T.ch[l];
                if (c == CHZ_NONE) {
                    CHECK(T.inc[l] == 0 && T.shift[l] == 0);
                    continue;
                }
                CHECK(c < g.n_ch && (l == 0 || T.ch[l - 1] != CHZ_NONE));
                if (c >= g.n_ch) continue;
                seen[c]++;
                n_of_kind++;
                CHECK(ch.kind[c] == k && ch.src[c] == source && lay.slot_of[c] == t * CHZ_TILE_CH + l);
                CHECK(T.inc[l] == (k == CHZ_TRACK ? (uint32_t)ch.trk[c] | (ch.trk_fresh[c] ? CHZ_TRACK_FRESH : 0u) : ch.inc[c]));
            }
        }
        CHECK(n_of_kind == ch.n_kind[k]);
        const ChzWgSet &w = lay.wg[k];
        CHECK(w.waves >= 1 && w.wpt >= 1 && w.waves * w.wpt <= CHZ_WAVES);
        for (const ChzWg &r : w.wgs) {
            CHECK(r.n_tiles >= 1 && r.n_tiles <= CHZ_WAVES && r.first_tile >= lay.first_tile[k] && r.first_tile + r.n_tiles <= lay.first_tile[k + 1]);
            if (k == CHZ_GAIN || k == CHZ_SCAN) CHECK(r.n_tiles <= w.waves);
            for (uint32_t t = r.first_tile; t < r.first_tile + r.n_tiles && t < n_tiles; t++) {
                covered[t]++;
                CHECK(lay.tiles[t].ch[0] != CHZ_NONE && ch.src[lay.tiles[t].ch[0]] == r.source && r.source < n_src);
            }
        }
        for (uint32_t t = 0; t < n_tiles; t++) CHECK(covered[t] == (t >= lay.first_tile[k] && t < lay.first_tile[k + 1] ? 1u : 0u));
    }
    for (uint32_t c = 0; c < g.n_ch; c++) CHECK(seen[c] == 1);
    // host-packed: the fixed and the gain tiles; the others' operands stay zero (their kernels build them)
    for (size_t i = lay.first_tile[CHZ_SCAN] * g.tile_bytes(); i < lay.amat.size(); i++)
        if (lay.amat[i]) {
            CHECK(!"operands of a tile that is not host-packed");
            break;
        }
}

// ---- upload pieces ------------------------------------------------------------------------------------------------------------

struct Sent {
    std::set<uint32_t> tiles[CHZ_WGS];             // per tile array: the tiles sent
    std::set<int> wgs;
    bool operator==(const Sent &o) const { return tiles[0] == o.tiles[0] && tiles[1] == o.tiles[1] && tiles[2] == o.tiles[2] && wgs == o.wgs; }
};

static Sent sent(const ChzGeometry &g, const ChzLayout &lay, const std::vector<ChzPiece> &pieces)
{
    Sent s;
    for (const ChzPiece &p : pieces) {
        CHECK(p.array >= 0 && p.array < CHZ_ARRAYS && (p.array != CHZ_GSUM || g.fmt == IQD_WIDE_S16));
        if (p.array < 0 || p.array >= CHZ_ARRAYS) continue;
        const size_t unit = p.array == CHZ_AMAT ? g.tile_bytes() : p.array == CHZ_TILES ? sizeof(ChzTile) : p.array == CHZ_GSUM ? sizeof(ChzFmtTile) : sizeof(ChzWg);
        // (the A operands: only the host-packed tiles' are ever sent)
        const size_t whole = p.array == CHZ_AMAT ? lay.first_tile[CHZ_SCAN] * g.tile_bytes() : lay.array(p.array).bytes;
        CHECK(p.bytes > 0 && p.offset % unit == 0 && p.bytes % unit == 0 && p.offset + p.bytes <= whole && whole <= lay.array(p.array).bytes);
        if (p.array >= CHZ_WGS) {
            CHECK(p.offset == 0 && p.bytes == whole && s.wgs.insert(p.array - CHZ_WGS).second);
            continue;
        }
        for (size_t t = p.offset / unit; t < (p.offset + p.bytes) / unit; t++) CHECK(s.tiles[p.array].insert((uint32_t)t).second);   // no tile twice
    }
    return s;
}

static void check_everything_sent(const ChzGeometry &g, const ChzLayout &lay, const std::vector<ChzPiece> &pieces)
{
    const Sent s = sent(g, lay, pieces);
    CHECK(s.tiles[CHZ_TILES].size() == lay.tiles.size() && s.tiles[CHZ_AMAT].size() == lay.first_tile[CHZ_SCAN]);
    CHECK(s.tiles[CHZ_GSUM].size() == (g.fmt == IQD_WIDE_S16 ? lay.tiles.size() : 0u) && lay.gsum.size() == s.tiles[CHZ_GSUM].size());
    for (int k = 0; k < CHZ_KINDS; k++) CHECK(s.wgs.count(k) == (lay.wg[k].wgs.empty() ? 0u : 1u));
}

// fmt IQD_WIDE_S16: fixed channels only (nothing follows on signed captures), and the row sums go with the tiles
static void check_pieces(uint32_t fmt)
{
    ChzGeometry g;
    ChzChannels ch;
    mixed_channels(g, ch, 2, 256, fmt);
    ChzLayout lay;
    bool regrouped = false;
    check_everything_sent(g, lay, lay.repack(g, ch, &regrouped));
    CHECK(regrouped && ch.any_dirty && ch.layout_dirty);                 // not clean before the caller says the pieces are queued:
    check_everything_sent(g, lay, lay.repack(g, ch, &regrouped));        // after a failed upload the same again
    CHECK(regrouped);
    ch.clean();
    CHECK(!ch.any_dirty && !ch.layout_dirty);
    CHECK(lay.repack(g, ch, &regrouped).empty() && !regrouped);          // nothing new: nothing to send
    for (int round = 0; round < 6; round++) {                            // single channels, neighbours, both ends
        std::set<uint32_t> chans;
        if (round == 0) chans = {0};
        if (round == 1) chans = {g.n_ch - 1};
        if (round == 2) chans = {0, g.n_ch - 1};
        for (uint32_t i = 0; round > 2 && i < (uint32_t)round; i++) chans.insert(rnd() % g.n_ch);
        Sent want;
        for (uint32_t c : chans) {
            const uint32_t t = lay.slot_of[c] / CHZ_TILE_CH;
            ch.inc[c] = rnd() << 8;
            ch.new_taps(g, c);
            want.tiles[CHZ_TILES].insert(t);
            if (t < lay.first_tile[CHZ_SCAN]) want.tiles[CHZ_AMAT].insert(t);
            if (fmt == IQD_WIDE_S16) want.tiles[CHZ_GSUM].insert(t);
        }
        const Sent s = sent(g, lay, lay.repack(g, ch, &regrouped));
        CHECK(!regrouped && s == want && ch.any_dirty);
        CHECK(sent(g, lay, lay.repack(g, ch, &regrouped)) == want);      // the same until clean()
        ch.clean();
        CHECK(lay.repack(g, ch, &regrouped).empty());
        for (uint32_t c : chans)
            if (ch.kind[c] != CHZ_TRACK) CHECK(lay.tiles[lay.slot_of[c] / CHZ_TILE_CH].inc[lay.slot_of[c] % CHZ_TILE_CH] == ch.inc[c]);
    }
    ch.src[3] ^= 1;                                                       // a source change: what set_channels does
    ch.layout_dirty = true;
    check_everything_sent(g, lay, lay.repack(g, ch, &regrouped));
    CHECK(regrouped);
    ch.clean();
    if (fmt == IQD_WIDE_S16) return;
    ch.set_kind(5, ch.kind[5] == CHZ_FIXED ? CHZ_GAIN : CHZ_FIXED);       // and a change of kind
    check_everything_sent(g, lay, lay.repack(g, ch, &regrouped));
    CHECK(regrouped);
}

int main()
{
    static const uint32_t KS[6] = {1, 31, 32, 33, 257, 1024};
    for (uint32_t q : {1u, 2u, 4u, 8u})
        for (uint32_t k : KS) {
            check_packing(q, k == 1024 ? 1024 * q : k, false);
            if (q == 1) check_packing(q, k, true);   // (the S16 sums: no fractional rate has them)
        }
    for (uint32_t n_src : {1u, 2u, 5u})
        for (uint32_t n_cus : {1u, 4u, 256u}) check_grouping(n_src, n_cus);
    check_pieces(IQD_WIDE_U8);
    check_pieces(IQD_WIDE_S16);
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("chan layout ok\n");
    return 0;
}
