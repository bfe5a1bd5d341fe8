// The channelizer object as its host code sees it (iqd_chan.cpp, iqd_chan_survey.cpp; nothing else includes this), the
// page-locked staging of its uploads and the staged form of a host call.
#pragma once
#include <string.h>

#include <initializer_list>

#include "iqd_chan_layout.h"
#include "iqd_hipres.h"

namespace iqd {

// Page-locked staging of a tap upload: the copies read it after the host call returned, so a slot is refilled only once
// the event behind its last copies has passed (two slots: the wait is for the upload before the previous one).
struct ChzStaging {
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

}  // namespace iqd

struct iqd_channelizer {
    iqd_t *e = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    iqd::ChzGeometry g;
    iqd::ChzChannels ch;
    iqd::ChzLayout lay;
    struct {                                      // the layout on the device, the tables, the stream's state
        iqd::DevBufExact lay[iqd::CHZ_ARRAYS];    // the twins of ChzLayout::array()
        iqd::DevBufExact phasor, proto, centre, hist[2];
    } d;
    int cur = 0;                                  // d.hist[cur]: the history the next call starts from
    uint64_t m_abs = 0;                           // outputs per channel since create / reset
    std::vector<unsigned long long> centre;       // [n_src]: source centre frequencies (the scan walker's)
    bool centre_dirty = true;
    struct {                                      // track following
        iqd_track_follow table{};                 // the track table in force (slots_dev NULL: none)
        iqd::DevBufExact carry[2], amat;          // the followers' carries (live, d) [n_ch], by call parity; large K: the scratch
        int cur = 0;
    } track;
    struct {                                      // the band survey: points measured on every source, in tiles of 8 of their own
        std::vector<uint32_t> inc;
        std::vector<iqd::ChzTile> tiles;          // ch[l]: the point index
        std::vector<uint8_t> amat;                // [n_tiles][q residues][nq][2][64][16]
        bool dirty = false;                       // packed, not uploaded yet
        iqd::DevBufExact d_amat, d_tiles;
    } sv;
    struct {                                      // uploads, and the host forms' device copies
        iqd::ChzStaging slot[2];
        int cur = 0;
        iqd::DevBufExact wide, out, sv_mag, rows, pcm, cnt, mag, sp;
    } stg;

    int fail(int code, const char *msg) { return iqd::engine_fail(e, code, msg); }
    hipError_t upload(const std::vector<iqd::ChzStaging::Piece> &pieces)   // through the next staging slot
    {
        hipError_t err = stg.slot[stg.cur].upload(pieces, stream);
        if (err == hipSuccess) stg.cur ^= 1;
        return err;
    }
};

#define CHZ_TRY(z, call)                                                                                  \
    do {                                                                                                  \
        hipError_t err_ = (call);                                                                         \
        if (err_ != hipSuccess) return (z)->fail(IQD_EHIP, hipGetErrorString(err_));                      \
    } while (0)

namespace iqd {

// One array of a host call: the caller's (NULL: none wanted), its bytes, the device copy, and which way it goes.
struct ChzStaged { const void *host; size_t bytes; DevBufExact *dev; bool out; };
constexpr bool CHZ_IN = false, CHZ_OUT = true;

// The host form of a call that has passed its check: every device copy is there before the first byte moves, so a failed
// allocation queues nothing; then the inputs go in, queue() - the call's own, on the device copies - queues its launches,
// the outputs come back and the call waits for them.  (Not counted in iqd_stats, unlike the band objects' copies.)
template <class Queue> int chz_staged_call(iqd_channelizer *z, std::initializer_list<ChzStaged> args, Queue queue)
{
    (void)hipSetDevice(z->device);
    for (const ChzStaged &a : args) CHZ_TRY(z, a.dev->ensure(a.bytes));
    for (const ChzStaged &a : args)
        if (!a.out && a.host) CHZ_TRY(z, hipMemcpyAsync(a.dev->p, a.host, a.bytes, hipMemcpyHostToDevice, z->stream));
    const int rc = queue();
    if (rc != IQD_OK) return rc;
    for (const ChzStaged &a : args)
        if (a.out && a.host) CHZ_TRY(z, hipMemcpyAsync(const_cast<void *>(a.host), a.dev->p, a.bytes, hipMemcpyDeviceToHost, z->stream));
    CHZ_TRY(z, hipStreamSynchronize(z->stream));
    return IQD_OK;
}

// iqd_chan.cpp, for the survey: the length rule of a capture, and what every launch of one call shares
int chz_check_len(iqd_channelizer *z, size_t bytes_per_source);
ChzLaunch chz_launch(const iqd_channelizer *z, const void *wide_dev, size_t bytes_per_source);

}  // namespace iqd
