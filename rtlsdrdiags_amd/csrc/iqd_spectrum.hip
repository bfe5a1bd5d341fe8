// Band spectrum (include/iqdemod.h: "Band spectrum"; layout of the operands: iqd_spectrum.h).
//
// The work is an int8 GEMM, bins x frames with K = 2 N bytes per frame.  A wave owns (source, block, tile of 16 bins) and
// takes the block's frames SPC_CHUNK at a time: SPC_FRAME_TILES MFMA tiles of 16 frames, each with four accumulators
// (rail r / i x low / high coefficient plane), so a K step of 64 bytes is 16 v_mfma_i32_16x16x64_i8 on four A operands
// (one 4 KiB contiguous read of the wave) and four B operands.  The B operand is the frame's interleaved bytes straight from the
// capture - lane (col, g) reads 16 bytes of frame col at K offset 16 g - flipped with ^ 0x80 for offset binary.  No LDS:
// frames do not overlap, so nothing is staged, and the A operands come from L2 per step (the four waves of a workgroup
// read the same frames and different bin tiles, so B is shared through the vector L1 and A is read once per wave).
//
// Epilogue, per lane (col, g) and tile: rows 4 g .. 4 g + 3 are four bins of frame col.  A = lo + 256 hi modulo 2^32,
// stage a, p = ar^2 + ai^2, summed per bin in 64 bits over the lane's frames; a frame past the block's end reads the
// block's last frame (never out of bounds) and adds nothing.  At the end the 16 columns are summed by shuffles and
// column 0 stores floor(sum / F) of its four bins as one 16-byte vector store.  A block is owned by one wave per bin
// tile: no atomics, no closing kernel, nothing to zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "iqd_chan_dev.h"
#include "iqd_spectrum.h"

namespace iqd {

// NT tiles of 16 frames from frame f0 of the block at blk (F frames of 2 n bytes); am: the bin tile's operands at this lane
template <bool FLIP, int NT>
__device__ __forceinline__ void spc_chunk(const uint8_t *blk, uint32_t n, uint32_t f0, uint32_t F, const uint4 *am,
                                          uint64_t (&sum)[4])
{
    const uint32_t lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const chz_v4i zero = {0, 0, 0, 0};
    chz_v4i acc[NT][SPC_PLANES];
    const uint8_t *bp[NT];
    bool valid[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const uint32_t f = f0 + 16 * t + col;
        valid[t] = f < F;
        bp[t] = blk + (size_t)min(f, F - 1) * (2 * n) + 16 * g;
#pragma unroll
        for (int p = 0; p < (int)SPC_PLANES; p++) acc[t][p] = zero;
    }
    const uint32_t steps = n / 32;
    for (uint32_t q = 0; q < steps; q++) {
        chz_v4i A[SPC_PLANES];
#pragma unroll
        for (int p = 0; p < (int)SPC_PLANES; p++) A[p] = __builtin_bit_cast(chz_v4i, am[(q * SPC_PLANES + p) * 64]);
#pragma unroll
        for (int t = 0; t < NT; t++) {
            uint4 v = *(const uint4 *)(bp[t] + 64 * q);
            if (FLIP) { v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u; }
            const chz_v4i b = __builtin_bit_cast(chz_v4i, v);
#pragma unroll
            for (int p = 0; p < (int)SPC_PLANES; p++)
                acc[t][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[p], b, acc[t][p], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // A = lo + 256 hi fits int32 (the window's bounds), 256 hi alone need not: combined modulo 2^32
            const int32_t Ar = (int32_t)((uint32_t)acc[t][0][r] + ((uint32_t)acc[t][1][r] << 8) + 32768u);
            const int32_t Ai = (int32_t)((uint32_t)acc[t][2][r] + ((uint32_t)acc[t][3][r] << 8) + 32768u);
            const int32_t ar = Ar >> 16, ai = Ai >> 16;              // |a| <= 23172
            const uint32_t p = (uint32_t)(ar * ar + ai * ai);         // < 2^31
            sum[r] += valid[t] ? p : 0u;
        }
}

template <bool FLIP>
__global__ __launch_bounds__(SPC_WAVES * 64) void spc_kernel(const SpcLaunch a)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, g = lane >> 4;
    const uint32_t n = a.n, F = a.frames, wgs_per_block = n / SPC_WG_BINS;
    uint32_t x = blockIdx.x;
    const uint32_t tile = (x % wgs_per_block) * SPC_WAVES + wave;       // of 16 bins
    x /= wgs_per_block;
    const uint32_t block = x % a.n_blocks, source = x / a.n_blocks;
    const uint8_t *blk = a.wide + (size_t)source * a.bytes_per_source + (size_t)block * F * (2 * n);
    const uint4 *am = a.amat + (size_t)tile * (n / 32) * SPC_PLANES * 64 + lane;

    uint64_t sum[4] = {0, 0, 0, 0};
    uint32_t f0 = 0;
    for (; f0 + SPC_CHUNK <= F; f0 += SPC_CHUNK) spc_chunk<FLIP, SPC_FRAME_TILES>(blk, n, f0, F, am, sum);
    const uint32_t rest = F - f0;                                        // < SPC_CHUNK
    if (rest > 32) {
        if (rest > 48) spc_chunk<FLIP, 4>(blk, n, f0, F, am, sum);
        else spc_chunk<FLIP, 3>(blk, n, f0, F, am, sum);
    } else if (rest > 0) {
        if (rest > 16) spc_chunk<FLIP, 2>(blk, n, f0, F, am, sum);
        else spc_chunk<FLIP, 1>(blk, n, f0, F, am, sum);
    }

    uint32_t out[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        uint64_t v = sum[r];
        v += (uint64_t)__shfl_xor((unsigned long long)v, 1);
        v += (uint64_t)__shfl_xor((unsigned long long)v, 2);
        v += (uint64_t)__shfl_xor((unsigned long long)v, 4);
        v += (uint64_t)__shfl_xor((unsigned long long)v, 8);
        out[r] = (uint32_t)(v / F);                                      // mean of values < 2^31
    }
    if (col == 0) {
        uint32_t *dst = a.power + ((size_t)source * a.n_blocks + block) * n + SPC_TILE_BINS * tile + 4 * g;
        *(uint4 *)dst = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

hipError_t launch_spectrum(const SpcLaunch &a, hipStream_t s)
{
    const uint64_t n_wgs = (uint64_t)a.n_sources * a.n_blocks * (a.n / SPC_WG_BINS);
    if (n_wgs == 0 || n_wgs > 0x7fffffffull || a.frames == 0) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)n_wgs), wg(SPC_WAVES * 64);
    if (a.flip) hipLaunchKernelGGL(spc_kernel<true>, grid, wg, 0, s, a);
    else hipLaunchKernelGGL(spc_kernel<false>, grid, wg, 0, s, a);
    return hipGetLastError();
}

}  // namespace iqd
