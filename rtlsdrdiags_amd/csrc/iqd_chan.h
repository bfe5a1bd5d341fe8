// Wideband channelizer (include/iqdemod.h: iqd_channelizer_*): launch descriptor of the gfx950 kernel and the host-only
// pieces of its integer spec, shared by iqd_chan.hip (device) and the host code (iqd_chan.cpp, iqd_chan_layout.cpp,
// iqd_chan_design.cpp, iqd_chan_survey.cpp).
//
// Per source the filter is a GEMM on v_mfma_i32_16x16x64_i8: A = (8 channels x {Ar, Ai}) x (2 Kp bytes of window),
// B = (2 Kp bytes) x (16 outputs), the sliding window over the source's interleaved signed bytes.  Kp = K rounded up to
// 32 samples (the taps of k >= K are 0), so that a window is a whole number of 64-byte K-chunks.  K-index kappa of a
// window (0 = oldest byte) is sample k = Kp - 1 - kappa / 2, rail kappa & 1 (I, Q).  Row 2 l + 0 of a tile (channel l)
// holds gr[k] on I and -gi[k] on Q, row 2 l + 1 gi[k] on I and gr[k] on Q; every int16 tap t = 256 hi + lo is split
// into two signed-byte planes, each plane one MFMA, combined exactly in the epilogue.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "iqdemod.h"
#include "iqd_device.h"

namespace iqd {

constexpr uint32_t CHZ_TILE_CH = 8;          // channels per 16-row MFMA tile (one wave)
constexpr uint32_t CHZ_WAVES = 8;            // tiles (waves) per workgroup, all of one source
constexpr uint32_t CHZ_GROUP = 64;           // outputs per store group: 8 channels x 128 bytes = one 16-byte store per lane
constexpr uint32_t CHZ_PHASOR = 4096;
constexpr uint32_t CHZ_WIN_MAX = 32768;      // LDS bytes of a workgroup's window
constexpr uint32_t CHZ_LDS_FIXED = CHZ_PHASOR * 4 + CHZ_WAVES * CHZ_TILE_CH * 2 * CHZ_GROUP;   // phasor + output staging
constexpr uint32_t CHZ_NQ_REG = 8;           // up to this many K-chunks the A operands stay in registers
constexpr uint32_t CHZ_NONE = 0xffffffffu;   // a padding slot of a tile
constexpr uint32_t CHZ_PROTO_MAX = 1024;     // prototype taps (the scan walker keeps them in LDS, zero up to Kp)
constexpr uint32_t CHZ_SCAN_MAGSUM = 2 * CHZ_WAVES * CHZ_TILE_CH * 4;   // the walker's per-block magnitude sums in LDS

// Fractional decimation P / Q (Q = 2, 4, 8; chz_frac_kernel): the outputs m = rho + Q t of one residue rho are an integer
// decimator by P (n = P t + floor(((rho + 1) P - 1) / Q)) with the tap set of branch ((rho + 1) P - 1) mod Q, so one MFMA
// tile is 16 outputs of one residue; amat is [n_tiles][Q residues][nq][2 planes][64 lanes] and a store group is
// chz_frac_group(Q) consecutive outputs, assembled from the Q residues in the wave's staging row.
constexpr uint32_t chz_frac_group(uint32_t q) { return 16 * (q < 4 ? 4 : q); }
constexpr uint32_t CHZ_FRAC_STAGE = CHZ_WAVES * CHZ_TILE_CH * 2 * chz_frac_group(8);   // the staging rows at Q = 8
constexpr uint32_t CHZ_FRAC_WIN_MAX = CHZ_WIN_MAX - (CHZ_FRAC_STAGE - CHZ_WAVES * CHZ_TILE_CH * 2 * CHZ_GROUP);   // same LDS in all

struct ChzTile {
    uint32_t ch[CHZ_TILE_CH];       // output row per slot, CHZ_NONE = padding (its taps are 0, nothing is stored)
    uint32_t inc[CHZ_TILE_CH];      // phase increment d_c
    uint32_t shift[CHZ_TILE_CH];    // gain shift L_c
};

struct ChzWg {                       // one workgroup row of the grid: up to CHZ_WAVES tiles of one source
    uint32_t source, first_tile, n_tiles, pad;
};

struct ChzLaunch {
    const uint8_t *wide;             // [n_sources][bytes_per_source] offset-binary I/Q, 16-byte aligned
    const uint8_t *hist;             // [n_sources][2 kp] raw bytes of samples [-kp, 0) of this call
    uint8_t *hist_next;              // the same after this call
    const uint32_t *phasor;          // [4096]: (uint16)c | s << 16
    const uint4 *amat;               // [n_tiles][den residues][nq][2 planes][64 lanes] A operands
    const ChzTile *tiles;
    const ChzWg *wgs;
    uint8_t *out;                    // [n_ch][out_row]
    size_t bytes_per_source;
    uint32_t n_sources, out_row, n_out, m, kp, nq, t_blk;   // m: M, or P of a fractional decimation; kp, nq: per branch
    uint32_t nbase;                  // (outputs before this call * M) mod 2^32; fractional: (outputs / Q) P mod 2^32
    uint32_t den;                    // Q of a fractional channelizer (decimation m / den), 1 otherwise
    uint32_t rail_bytes;             // B, bytes per rail of wide / hist: 1 (U8, S8) or 2 (S16); the history is 2 kp B bytes
};

// What a walker (chz_scan_kernel, chz_gain_kernel) reads besides ChzLaunch: a.wgs are its own workgroups (tiles of its
// kind of following channels only); the engine's per-channel state is read, never written (the walker steps a shadow copy).
struct ChzWalkLaunch {
    const AgcConfig *agc_cfg;              // the engine's state, [engine ch]
    const AgcState *agc;
    const Consts *consts;                  // the engine's constant tables (dB table)
    uint32_t first_ch;                     // engine channel of channelizer channel 0
    uint32_t block_out, n_blocks;          // outputs per block, blocks in this call
    uint32_t t_blk;                        // outputs per window (a multiple of 64, or the whole short block)
    uint32_t waves;                        // tiles per workgroup
    uint32_t wpt;                          // waves per tile (waves * wpt <= CHZ_WAVES)
};
// the scan walker's (chz_scan_kernel) besides
struct ChzScanLaunch : ChzWalkLaunch {
    const int16_t *proto;                  // [kp] prototype, zero from K on
    const unsigned long long *centre;      // [n_sources] source centre frequencies F_s
    const ChanParams *params;              // the engine's state, [engine ch]
    const ScanConfig *scan_cfg;
    const ScanState *scan;
    const uint32_t *tracker;
};

// The gain walker (chz_gain_kernel, iqd_chan_gain.hip) reads nothing besides: its tiles' A operands are host-packed like
// the fixed ones.
struct ChzGainShadow { AgcConfig cfg; AgcState st; };
constexpr uint32_t CHZ_GAIN_SHADOW = CHZ_WAVES * CHZ_TILE_CH * (uint32_t)sizeof(ChzGainShadow);   // the walker's shadows in LDS
struct ChzGainLaunch : ChzWalkLaunch {};

// Track-following channels (chz_track_kernel, iqd_chan_track.hip) beside ChzLaunch: a.wgs are the track tiles' workgroup
// rows, a.t_blk the outputs of one window of a block.  ChzTile::inc of a track tile is not an increment: it holds the table
// slot its channel follows, and CHZ_TRACK_FRESH while the channel's carry does not count (it has just started to follow).
constexpr uint32_t CHZ_TRACK_FRESH = 0x80000000u;
constexpr size_t CHZ_TRACK_SCRATCH = (size_t)64 << 20;   // large K: the most bytes of per-(block, tile) A operands of one run of
                                                         // blocks (one block's, where that alone is more)
struct ChzTrackLaunch {
    const iqd_track_slot *slots;           // [n_sources][n_blocks][n_slots], read when the kernel runs
    const uint2 *carry;                    // [n_ch]: (live, d) the previous call left (block 0 at lag 1)
    uint2 *carry_next;                     // the same after this call: the decision of table block n_blocks - 1
    const int16_t *proto;                  // [kp] prototype, zero from K on
    uint4 *amat;                           // nq > CHZ_NQ_REG: [blocks of a run][n_tiles][nq][2 planes][64 lanes]
    uint32_t n_slots, n_blocks;            // S and the blocks per source of the table
    uint32_t block_out;                    // outputs per table block, a multiple of 32
    uint32_t wins;                         // windows per block, ceil(block_out / a.t_blk)
    uint32_t lag, min_state;
    uint32_t b0;                           // first table block of this launch (a run of the large-K path; else 0)
    uint32_t first_tile, n_tiles;          // the track tiles are [first_tile, first_tile + n_tiles) of a.tiles
};

// The band survey (chz_survey_kernel, iqd_chan_survey.hip) beside ChzLaunch: a.tiles / a.amat are the survey's point tiles
// (ChzTile::ch is the point index), shared by all sources; a.wgs and a.out are unused.  Workgroup x of the grid is
// (source, window, row of CHZ_WAVES point tiles) = (x / (n_win rows), x / rows % n_win, x % rows).
struct ChzSurveyLaunch {
    uint32_t *sums;                        // [n_sources][n_blocks][n_points], zero before the launch; the result after it
    uint32_t n_points, n_tiles;            // n_tiles = ceil(n_points / 8)
    uint32_t n_blocks, block_out;          // blocks per row, outputs per block (n_blocks block_out = a.n_out)
    uint32_t n_win, rows;                  // windows of a.t_blk outputs per source; ceil(n_tiles / CHZ_WAVES)
};

// Signed captures (chz_fmt_kernel, iqd_chan_fmt.hip; IQD_WIDE_S8 / IQD_WIDE_S16) beside ChzLaunch, whose fields mean what
// they mean to chz_kernel except: a.wide / a.hist / a.hist_next are raw capture bytes of the format (2 B bytes per sample,
// B = a.rail_bytes: 1 is S8, one plane; 2 is S16, planes hi and lo'; zero history is zero bytes) and a.bytes_per_source
// counts them.  The window is staged as B signed-byte planes of 2 (t_blk m + kp) bytes each, pstride apart.
struct ChzFmtTile {
    int32_t g[CHZ_TILE_CH][2];             // per slot: the coefficient sums of its rows, sum gr - sum gi and sum gr + sum gi
};
struct ChzFmtLaunch {
    ChzLaunch a;
    const ChzFmtTile *gsum;                // [n_tiles], beside a.tiles (S16 only)
    uint32_t pstride;                      // LDS bytes from one plane to the next: >= 2 (t_blk m + kp) + 16, a multiple of 16
};

// The most outputs of one window at decimation m / q with `rail` byte planes of the samples in LDS (1: U8 and S8, 2: S16):
// 2 rail (t m / q + kp) <= CHZ_WIN_MAX (q > 1: CHZ_FRAC_WIN_MAX), whole store groups, at most 1024.
// (iqd_channelizer_window_outputs exports it.)
constexpr uint32_t chz_window_outputs(uint32_t m, uint32_t kp, uint32_t q, uint32_t rail)
{
    const uint32_t group = q > 1 ? chz_frac_group(q) : CHZ_GROUP;
    const uint64_t t = (uint64_t)((q > 1 ? CHZ_FRAC_WIN_MAX : CHZ_WIN_MAX) / (2 * rail) - kp) * q / m;
    return (uint32_t)(t < 1024 ? t : 1024) / group * group;
}

// The same for a track follower's window, which shares the LDS with the prototype (2 CHZ_PROTO_MAX bytes):
// 2 (t m + kp) <= CHZ_WIN_MAX - 2 CHZ_PROTO_MAX.  (iqd_channelizer_track_window_outputs exports it.)
constexpr uint32_t chz_track_window_outputs(uint32_t m, uint32_t kp)
{
    const uint32_t t = ((CHZ_WIN_MAX - 2 * CHZ_PROTO_MAX) / 2 - kp) / m;
    return (t < 1024 ? t : 1024) / CHZ_GROUP * CHZ_GROUP;
}

// iqd_channelizer_tuning: the increment of a channel whose station is `station` Hz (centre station + 64000 r) cut from a
// source centred on `centre` Hz at Fs = 256000 M; false when out of band.  Host and device share this one statement.
__host__ __device__ inline bool chz_tuning(uint32_t m, unsigned long long centre, unsigned long long station, int32_t r,
                                           uint32_t *inc)
{
    const __int128 fs = (__int128)256000 * m;
    const __int128 o = (__int128)station + (__int128)(64000 * r) - (__int128)centre;
    if (o < -(fs / 2) || o >= fs / 2) return false;
    // floor((o 2^32 + Fs/2) / Fs) on a non-negative numerator: (o + Fs/2) 2^32 + Fs/2 < 2^56 gives the quotient + 2^31
    const unsigned long long num = ((unsigned long long)(o + fs / 2) << 32) + (unsigned long long)(fs / 2);
    *inc = (uint32_t)(num / (unsigned long long)fs) ^ 0x80000000u;
    return true;
}

// One call: n_fixed_wgs workgroups of the fixed channels' kernel (a.wgs; chz_frac_kernel when a.den > 1, else chz_kernel),
// n_scan_wgs of the walker (scan_wgs, with scan; none: 0 and NULL), then the history kernel
hipError_t launch_channelizer(const ChzLaunch &a, uint32_t n_fixed_wgs, const ChzWg *scan_wgs, uint32_t n_scan_wgs,
                              const ChzScanLaunch *scan, hipStream_t st);
// chz_history_kernel alone: the last 2 a.kp a.rail_bytes bytes of [history | this call] per source into a.hist_next
hipError_t launch_channelizer_history(const ChzLaunch &a, hipStream_t st);
// chz_frac_kernel alone, for a.den = 2, 4, 8 (iqd_chan_frac.hip); launch_channelizer adds the history kernel
hipError_t launch_channelizer_frac(const ChzLaunch &a, uint32_t n_wgs, hipStream_t s);
// chz_survey_kernel for a.den = 1, 2, 4, 8 and the kernel that divides the sums (iqd_chan_survey.hip)
hipError_t launch_channelizer_survey(const ChzLaunch &a, const ChzSurveyLaunch &s, hipStream_t st);

// chz_fmt_kernel for f.a.rail_bytes = 1, 2 (iqd_chan_fmt.hip) and the history kernel
hipError_t launch_channelizer_fmt(const ChzFmtLaunch &f, uint32_t n_wgs, hipStream_t st);

// chz_gain_kernel alone: n_wgs workgroups a.wgs of gain-following tiles, one launch whatever g.n_blocks (iqd_chan_gain.hip)
hipError_t launch_channelizer_gain(const ChzLaunch &a, uint32_t n_wgs, const ChzGainLaunch &g, hipStream_t st);

// chz_track_kernel alone: n_wgs workgroup rows a.wgs of track tiles.  nq <= CHZ_NQ_REG: one launch whatever t.n_blocks; else
// per run of run_blocks table blocks chz_track_build_kernel and chz_track_kernel<0> (iqd_chan_track.hip)
hipError_t launch_channelizer_track(const ChzLaunch &a, uint32_t n_wgs, const ChzTrackLaunch &t, uint32_t run_blocks, hipStream_t st);

// host-only spec pieces (iqd_chan_design.cpp)
void chz_phasor_table(int16_t *out /* [8192] (c, s) pairs */);
// complex taps of one channel: gr, gi [K] (iqd_chan_layout.cpp)
void chz_channel_taps(const int16_t *h, uint32_t k, uint32_t inc, const int16_t *phasor, int16_t *gr, int16_t *gi);

// the engine's side (iqd_engine.cpp)
int engine_fail(iqd_t *e, int code, const char *msg);
void engine_geometry(const iqd_t *e, uint32_t *n_ch, uint32_t *block_bytes, uint32_t *flags);
// Applies the pending settings now (parameters, AGC one-shots, the scanner's start jump: once; the accept that follows
// finds nothing left to apply) and fills the device state pointers of s.
int engine_settle(iqd_t *e, ChzScanLaunch *s);

}  // namespace iqd
