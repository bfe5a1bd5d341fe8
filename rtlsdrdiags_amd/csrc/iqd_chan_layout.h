// Wideband channelizer, host side: what needs no GPU.  The geometry a create fixes, the channels and their taps, and the
// layout made of them - the channels grouped by kind and source into tiles of 8, the tiles' taps packed as MFMA A operands
// (iqd_chan.h), the workgroup rows of each kind's kernel, and which parts of all that an upload has to send.  No HIP call
// here or in iqd_chan_layout.cpp / iqd_chan_design.cpp (tests/chan_layout builds the two alone, on the CPU).
#pragma once
#include <vector>

#include "iqd_chan.h"

namespace iqd {

// the four kinds of channel: each has tiles and workgroups of its own and its kernel.  A tile's kind follows from its
// index: tiles [first_tile[k], first_tile[k + 1]) hold kind k, so the host-packed ones are those below first_tile[CHZ_SCAN]
// (a scanner- or track-following channel's kernel builds its operands itself, per block).
enum { CHZ_FIXED, CHZ_GAIN, CHZ_SCAN, CHZ_TRACK, CHZ_KINDS };

struct ChzGeometry {
    uint32_t n_src = 0, n_ch = 0, m = 0, k = 0, kp = 0, nq = 0;
    uint32_t q = 1, kb = 0;                       // decimation m / q; kb = ceil(k / q), the longest branch
    uint32_t fmt = IQD_WIDE_U8, rail = 1;         // sample format of the captures; bytes per rail B (2: IQD_WIDE_S16)
    uint32_t n_cus = 256;
    std::vector<int16_t> h, phasor;               // prototype [K]; (c, s) pairs [8192]

    ChzGeometry() = default;
    ChzGeometry(const iqd_channelizer_config &cfg, std::vector<int16_t> taps);
    // bytes of one channel's row for bytes_per_source capture bytes
    size_t row_bytes(size_t bytes_per_source) const { return bytes_per_source / ((size_t)m * rail) * q; }
    size_t tile_bytes() const { return (size_t)q * nq * 2 * 64 * 16; }      // one tile's A operands
    size_t taps_per_channel() const { return (size_t)q * kb; }
    uint32_t t_max() const { return chz_window_outputs(m, kp, q, rail); }   // the most outputs of one window
};

struct ChzChannels {
    std::vector<uint32_t> src, inc;
    std::vector<uint8_t> shift;
    std::vector<uint8_t> kind;                    // [n_ch]: CHZ_FIXED .. CHZ_TRACK
    uint32_t n_kind[CHZ_KINDS] = {};
    std::vector<int32_t> trk;                     // [n_ch]: the table slot a CHZ_TRACK channel follows, -1 otherwise
    std::vector<uint8_t> trk_fresh;               // [n_ch]: it has started to follow since the last call (its carry does not count)
    bool any_fresh = false;
    std::vector<int16_t> gr, gi;                  // [n_ch][q branches][kb], zero from a branch's length on
    bool layout_dirty = true;                     // a channel changed source or kind: regroup
    std::vector<uint8_t> ch_dirty;                // new taps since the last packing
    bool any_dirty = true;

    void create(const ChzGeometry &g);
    void new_taps(const ChzGeometry &g, uint32_t c);   // after inc[c] changed
    void set_kind(uint32_t c, int k);
    void clean();                                 // what ChzLayout::repack listed has been queued: nothing is dirty
};

struct ChzWgSet {
    std::vector<ChzWg> wgs;
    uint32_t waves = 1, wpt = 1;                  // a walker's: tiles per workgroup, waves per tile
};

// the layout's arrays, each with a twin on the device: the A operands, the tiles, the S16 sums, every kind's workgroup rows
enum { CHZ_AMAT, CHZ_TILES, CHZ_GSUM, CHZ_WGS /* + the kind */, CHZ_ARRAYS = CHZ_WGS + CHZ_KINDS };
struct ChzSpan { const void *p; size_t bytes; };
// one copy of an upload: `bytes` from `offset` of a host array to the same offset of its device twin
struct ChzPiece { int array; size_t offset, bytes; };

struct ChzLayout {
    std::vector<ChzTile> tiles;
    uint32_t first_tile[CHZ_KINDS + 1] = {};
    ChzWgSet wg[CHZ_KINDS];                       // chz_kernel's workgroups (fixed channels), the gain walker's, the scan walker's, chz_track_kernel's
    std::vector<uint32_t> slot_of;                // [n_ch]: tile * 8 + slot
    std::vector<uint8_t> amat;                    // [n_tiles][q residues][nq][2][64][16]
    std::vector<ChzFmtTile> gsum;                 // [n_tiles]: the rows' coefficient sums (IQD_WIDE_S16 only)

    ChzSpan array(int a) const;                   // a of CHZ_AMAT .. CHZ_WGS + kind
    void group(const ChzGeometry &g, const ChzChannels &ch);
    // Regroups where a channel changed source or kind, packs the slots of the channels with new parameters and lists what
    // to send: runs of consecutive tiles with such a slot as one piece per array (after a regrouping, everything, the
    // workgroup rows too).  *regrouped: the arrays may have grown.  The channels stay dirty until ChzChannels::clean(), which
    // the caller makes once the pieces have been queued: after a failed upload the next repack lists the same again.
    std::vector<ChzPiece> repack(const ChzGeometry &g, const ChzChannels &ch, bool *regrouped);
};

// complex taps of increment inc on every branch, gr / gi [q][kb]
void chz_branch_taps(const ChzGeometry &g, uint32_t inc, int16_t *gr, int16_t *gi);
// One slot l of tile `tile`: its ChzTile entries (ch CHZ_NONE: padding, all zero) and, where amat is not NULL, its A operands
// from the taps gr / gi [q][kb]; where gsum is not NULL, its rows' coefficient sums as well.
void chz_pack_slot(const ChzGeometry &g, ChzTile &t, uint32_t tile, uint32_t l, uint32_t ch, uint32_t inc, uint32_t shift,
                   const int16_t *gr, const int16_t *gi, uint8_t *amat, ChzFmtTile *gsum);

// iqd_chan_design.cpp.  Q in {1, 2, 4, 8}, gcd(P, Q) = 1 (P odd when Q > 1), 2 <= P / Q <= 64
bool chz_ratio_ok(uint32_t p, uint32_t q);

}  // namespace iqd
