// Wideband channelizer, host side: the band survey (include/iqdemod.h: iqd_channelizer_set_survey, iqd_channelizer_survey*).
// The points are packed like channels, in tiles of 8 of their own that every source shares, and go to chz_survey_kernel
// (iqd_chan_survey.hip) with the history read only: a survey looks and does not touch.
#include <algorithm>

#include "iqd_chan_impl.h"

using namespace iqd;

// every refusal of a survey, in order; the alignment is the device form's
static int survey_check(iqd_channelizer *z, const void *wide, size_t bytes_per_source, uint32_t block_bytes, const void *magnitude, bool device)
{
    if (!wide || !magnitude) return z->fail(IQD_EINVAL, "channelizer: NULL buffer");
    if (device && ((((uintptr_t)wide) | ((uintptr_t)magnitude)) & 15)) return z->fail(IQD_EINVAL, "channelizer: buffers must be 16-byte aligned");
    if (z->sv.inc.empty()) return z->fail(IQD_EINVAL, "channelizer: no survey points set");
    if (z->ch.n_kind[CHZ_SCAN]) return z->fail(IQD_EINVAL, "channelizer: no survey while a channel follows its scanner");
    if (z->ch.n_kind[CHZ_GAIN]) return z->fail(IQD_EINVAL, "channelizer: no survey while a channel follows its gain");
    if (z->ch.n_kind[CHZ_TRACK]) return z->fail(IQD_EINVAL, "channelizer: no survey while a channel follows a track slot");
    int rc = chz_check_len(z, bytes_per_source);
    if (rc != IQD_OK) return rc;
    const ChzGeometry &g = z->g;
    const uint32_t unit = g.q > 1 ? 256 : 64;
    if (block_bytes == 0 || block_bytes % unit != 0 || block_bytes > (1u << 24))
        return z->fail(IQD_EINVAL, g.q > 1 ? "channelizer: a survey's block_bytes must be a multiple of 256, at most 2^24"
                                           : "channelizer: a survey's block_bytes must be a multiple of 64, at most 2^24");
    const size_t row = bytes_per_source / g.m * g.q;
    if (row % block_bytes != 0) return z->fail(IQD_EINVAL, "channelizer: a survey's block_bytes must divide the row length");
    const uint64_t n_res = (uint64_t)g.n_src * (row / block_bytes) * z->sv.inc.size();
    const uint32_t n_out = (uint32_t)(row / 2), t_blk = std::min(n_out, g.t_max());
    const uint64_t n_wgs = (uint64_t)g.n_src * ((n_out + t_blk - 1) / t_blk) * ((z->sv.tiles.size() + CHZ_WAVES - 1) / CHZ_WAVES);
    if (n_res > 0x3fffffffull || n_wgs > 0x7fffffffull) return z->fail(IQD_EINVAL, "channelizer: survey too large for one call");
    return IQD_OK;
}

// a checked survey onto the stream: the point tiles (through a staging slot, like the channels' taps) if they are new, the
// zeros, the kernel
static int survey_queue(iqd_channelizer *z, const void *wide_dev, size_t bytes_per_source, uint32_t block_bytes, void *magnitude_dev)
{
    (void)hipSetDevice(z->device);
    if (z->sv.dirty) {
        const size_t ab = z->sv.amat.size(), tb = z->sv.tiles.size() * sizeof(ChzTile);
        CHZ_TRY(z, z->sv.d_amat.ensure(ab));
        CHZ_TRY(z, z->sv.d_tiles.ensure(tb));
        CHZ_TRY(z, z->upload({{z->sv.d_amat.p, z->sv.amat.data(), ab}, {z->sv.d_tiles.p, z->sv.tiles.data(), tb}}));
        z->sv.dirty = false;
    }
    ChzLaunch a = chz_launch(z, wide_dev, bytes_per_source);
    a.amat = z->sv.d_amat.as<uint4>();
    a.tiles = z->sv.d_tiles.as<ChzTile>();
    ChzSurveyLaunch s{};
    s.sums = (uint32_t *)magnitude_dev;
    s.n_points = (uint32_t)z->sv.inc.size();
    s.n_tiles = (uint32_t)z->sv.tiles.size();
    s.block_out = block_bytes / 2;
    s.n_blocks = a.n_out / s.block_out;
    s.n_win = (a.n_out + a.t_blk - 1) / a.t_blk;
    s.rows = (s.n_tiles + CHZ_WAVES - 1) / CHZ_WAVES;
    CHZ_TRY(z, hipMemsetAsync(magnitude_dev, 0, (size_t)z->g.n_src * s.n_blocks * s.n_points * 4, z->stream));
    CHZ_TRY(z, launch_channelizer_survey(a, s, z->stream));
    return IQD_OK;
}

extern "C" {

int iqd_channelizer_set_survey(iqd_channelizer_t *z, uint32_t n_points, const uint32_t *phase_inc, const uint8_t *gain_shift)
{
    if (!z) return IQD_EINVAL;
    const ChzGeometry &g = z->g;
    if (n_points > 4096) return z->fail(IQD_EINVAL, "channelizer: a survey has at most 4096 points");
    if (n_points && g.fmt != IQD_WIDE_U8)
        return z->fail(IQD_EINVAL, g.fmt == IQD_WIDE_S16 ? "channelizer: the band survey of IQD_WIDE_S16 captures is not built yet"
                                                         : "channelizer: the band survey of IQD_WIDE_S8 captures is not built yet");
    if (n_points && !phase_inc) return z->fail(IQD_EINVAL, "channelizer: NULL survey increments");
    for (uint32_t i = 0; gain_shift && i < n_points; i++)
        if (gain_shift[i] > 8) return z->fail(IQD_EINVAL, "channelizer: gain shift must be 0..8");
    z->sv.inc.assign(phase_inc, phase_inc + n_points);
    const uint32_t n_tiles = (n_points + CHZ_TILE_CH - 1) / CHZ_TILE_CH;
    z->sv.tiles.assign(n_tiles, ChzTile{});
    z->sv.amat.assign(n_tiles * g.tile_bytes(), 0);
    std::vector<int16_t> gr(g.taps_per_channel()), gi(g.taps_per_channel());
    for (uint32_t p = 0; p < n_tiles * CHZ_TILE_CH; p++) {
        const bool pad = p >= n_points;
        std::fill(gr.begin(), gr.end(), 0);
        std::fill(gi.begin(), gi.end(), 0);
        if (!pad) chz_branch_taps(g, phase_inc[p], gr.data(), gi.data());
        chz_pack_slot(g, z->sv.tiles[p / CHZ_TILE_CH], p / CHZ_TILE_CH, p % CHZ_TILE_CH, pad ? CHZ_NONE : p, pad ? 0 : phase_inc[p],
                      !pad && gain_shift ? gain_shift[p] : 0, gr.data(), gi.data(), z->sv.amat.data(), nullptr);
    }
    z->sv.dirty = n_points != 0;
    return IQD_OK;
}

int iqd_channelizer_survey_device(iqd_channelizer_t *z, const void *wide_dev, size_t bytes_per_source, uint32_t block_bytes,
                                  void *magnitude_dev)
{
    if (!z) return IQD_EINVAL;
    int rc = survey_check(z, wide_dev, bytes_per_source, block_bytes, magnitude_dev, true);
    return rc != IQD_OK ? rc : survey_queue(z, wide_dev, bytes_per_source, block_bytes, magnitude_dev);
}

int iqd_channelizer_survey(iqd_channelizer_t *z, const uint8_t *wide, size_t bytes_per_source, uint32_t block_bytes, uint32_t *magnitude)
{
    if (!z) return IQD_EINVAL;
    int rc = survey_check(z, wide, bytes_per_source, block_bytes, magnitude, false);
    if (rc != IQD_OK) return rc;
    const size_t ob = (size_t)z->g.n_src * (bytes_per_source / z->g.m * z->g.q / block_bytes) * z->sv.inc.size() * 4;
    return chz_staged_call(z, {{wide, z->g.n_src * bytes_per_source, &z->stg.wide, CHZ_IN}, {magnitude, ob, &z->stg.sv_mag, CHZ_OUT}},
                           [&] { return survey_queue(z, z->stg.wide.p, bytes_per_source, block_bytes, z->stg.sv_mag.p); });
}

}  // extern "C"
