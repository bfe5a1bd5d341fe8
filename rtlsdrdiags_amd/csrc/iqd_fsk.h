// PCM packet decoder (include/iqdemod_fsk.h): what iqd_fsk.cpp and iqd_fsk.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace iqd {

constexpr uint32_t FSK_MIN_W = 2, FSK_MAX_W = 64, FSK_MAX_LEN = 1024, FSK_MAX_WINDOW = 32512;
constexpr uint32_t FSK_TILE = 256;             // samples of one channel a decision workgroup takes at a time: four waves of 64
constexpr uint32_t FSK_HIST = FSK_MAX_W;       // int16 per channel of carried samples (W - 1 used)
constexpr uint32_t FSK_BUF_BYTES = 1040;       // a channel's bit buffer: 8 max_len + 8 bits at most, in whole uint32
constexpr uint32_t FSK_RECORD_BYTES = 24, FSK_STATE_BYTES = 40;
constexpr size_t FSK_MAX_N = 0x7fffffffull;

// one channel's carried state (iqd_fsk_state's bytes)
struct FskState {
    uint64_t samples;
    uint32_t ph, prev, last, ones, in_frame, nbits, bad_fcs, frames_total;
};

// the header's sizes; b + g < 1.5 x 2^31 and n < 2^31: the product stays below 2^63
constexpr uint64_t fsk_maxbits(uint64_t n, uint32_t b, uint32_t shift) { return n ? ((n * ((uint64_t)b + (b >> shift))) >> 32) + 1 : 0; }

struct FskLaunch {
    // the object's
    int8_t coef[4][FSK_MAX_W];   // cm, sm, cs, ss; zeros from W on
    FskState *state;             // [n_channels]
    int16_t *hist;               // [n_channels][FSK_HIST]: the stream's last W - 1 samples, oldest first
    uint32_t *buf;               // [n_channels][FSK_BUF_BYTES / 4]: the bit buffer
    uint32_t *dec;               // scratch [n_channels][Dw]: the decisions, sample j of the call at word j / 32, bit j mod 32
    uint32_t n_channels, W, baud_inc, loop_shift, nrzi, min_len, max_len;
    // the call's
    const int16_t *pcm;
    const uint32_t *count;       // or NULL
    size_t row_stride;
    uint32_t n, Dw;              // Dw = ceil(n / 32)
    uint32_t F, Bw, Bc;          // the header's sizes for n
    uint32_t *n_bits, *bits;     // bits or NULL
    uint32_t *n_frames;
    uint32_t *frames;            // [n_channels][F] records of six uint32
    uint8_t *bytes;
};
hipError_t launch_fsk_decide(const FskLaunch &a, hipStream_t s);   // the decision words; n >= 1
hipError_t launch_fsk_walk(const FskLaunch &a, hipStream_t s);     // clock, NRZI, deframer, every output, the state

}  // namespace iqd
