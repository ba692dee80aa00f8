// q8_gemm_device.h -- the body every multi-row product on int8 group-quantized weights shares (q8_gemm.hip: the prompt
// pass's GEMM; q8_batch.hip: the batched step's q | k | v and classifier launches): one block of eight
// waves, 16 weight rows against up to NT tiles of 16 token rows on the int8 matrix cores.  One arithmetic: the bits of a
// (token row, weight row) product are the same through every kernel built on it.  Anonymous namespace, like q8_device.h.
//
// Both operands are K-contiguous int8 rows, so a lane's MFMA operand is one load from either matrix: the weight rows are
// the A side (the tile's 16 rows), the token rows the B side (its 16 columns).  One MFMA into a zeroed tile is exactly one
// group's I for 16 x 16 (row, token) pairs -- v_mfma_i32_16x16x64_i8 at group size 64 (16 bytes a lane from either
// matrix), v_mfma_i32_16x16x32_i8 at 32 (8 bytes) --, so a group never shares an MFMA with another and K is any whole
// number of groups.  The result tile has the token on the lane (lane & 15) and four consecutive weight rows in its
// registers (4 (lane >> 4) + r): after each group the four int32 are converted, scaled by their rows' ws[g] and the
// token's xs[g] -- (f32(I) * ws) * xs, the decode's order, the second product fused into the sum -- and added to the
// lane's four f32 sums.  The waves split K: wave w takes groups w, w + 8, ... in increasing order, leaves its sums in LDS
// (q8_gemm_stash), and the eight sums of a tile are then added in wave order 0 .. 7 (q8_gemm_tile_sum).
#pragma once
#include "q8_device.h"

namespace l2z {
namespace {

constexpr int kQgWaves = 8;               // K ranges of a block, one a wave
constexpr int kQgBlock = kQgWaves * kWave;
constexpr int kQgBatch = 4;               // groups a wave requests before it multiplies the first

template <int GS> struct Q8Frag;
template <> struct Q8Frag<64> {
    typedef v4i T;
    static __device__ __forceinline__ T zero() { return v4i{0, 0, 0, 0}; }
    static __device__ __forceinline__ v4i mfma(T a, T b) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, v4i{0, 0, 0, 0}, 0, 0, 0); }
};
template <> struct Q8Frag<32> {
    typedef long T;
    static __device__ __forceinline__ T zero() { return 0; }
    static __device__ __forceinline__ v4i mfma(T a, T b) { return __builtin_amdgcn_mfma_i32_16x16x32_i8(a, b, v4i{0, 0, 0, 0}, 0, 0, 0); }
};

// This wave's K range of a block's products -> acc[j], tile j's four sums of this lane.
// ap: the lane's weight row at its bytes of group 0 (a_in: the row lies in the matrix; else zeros are multiplied);
// wsp: group 0's scale of the lane's first output row, the rows ng apart; bp / xsp: the lane's token row of the block's
// first tile, likewise, the tiles 16 rows apart; nt <= NT: the block's tiles (block-uniform)
template <int GS, int NT>
__device__ __forceinline__ void q8_gemm_wave_sums(const int8_t *ap, bool a_in, const float *wsp, const int8_t *bp,
                                                  const float *xsp, int n, int nt, int wave, v4f (&acc)[NT])
{
    typedef typename Q8Frag<GS>::T Frag;
    const int ng = n / GS;
#pragma unroll
    for (int j = 0; j < NT; j++) acc[j] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    for (int g0 = wave; g0 < ng; g0 += kQgWaves * kQgBatch) {
        Frag wa[kQgBatch];
        v4f wsc[kQgBatch];
#pragma unroll
        for (int u = 0; u < kQgBatch; u++) {
            const int g = g0 + kQgWaves * u;
            const bool in = g < ng;  // (wave-uniform)
            wa[u] = (in && a_in) ? __builtin_nontemporal_load((const Frag *)(ap + (size_t)(in ? g : 0) * GS)) : Q8Frag<GS>::zero();
            const int gg = in ? g : 0;
            wsc[u] = v4f{wsp[gg], wsp[ng + gg], wsp[2 * ng + gg], wsp[3 * ng + gg]};
        }
        // Straight-line, so that the batch's token loads are all requested before the first MFMA waits for one: a group
        // past the row end multiplies the zero fragment against group 0 (its terms are +0: the sums keep their bits), a
        // tile past the chunk's last is tile 0 again (its sums are never stored)
#pragma unroll
        for (int u = 0; u < kQgBatch; u++) {
            const int g = g0 + kQgWaves * u < ng ? g0 + kQgWaves * u : 0;
#pragma unroll
            for (int j = 0; j < NT; j++) {
                const int jj = j < nt ? j : 0;
                const Frag xb = *(const Frag *)(bp + (size_t)jj * kQ8GemmTile * (size_t)n + (size_t)g * GS);
                const float xs = xsp[(size_t)jj * kQ8GemmTile * (size_t)ng + g];
                const v4i I = Q8Frag<GS>::mfma(wa[u], xb);
                const v4f p = v4f{(float)I.x, (float)I.y, (float)I.z, (float)I.w} * wsc[u];
                acc[j] = __builtin_elementwise_fma(p, v4f{xs, xs, xs, xs}, acc[j]);
            }
        }
    }
}

// the wave's sums -> part [kQgWaves * NT * kWave] in LDS, and the barrier behind them
template <int NT>
__device__ __forceinline__ void q8_gemm_stash(v4f *part, const v4f (&acc)[NT], int wave, int lane)
{
#pragma unroll
    for (int j = 0; j < NT; j++) part[(wave * NT + j) * kWave + lane] = acc[j];
    __syncthreads();
}

// the K ranges' sums of tile j for this lane, added in wave order
template <int NT>
__device__ __forceinline__ v4f q8_gemm_tile_sum(const v4f *part, int j, int lane)
{
    v4f v = part[j * kWave + lane];
#pragma unroll
    for (int w = 1; w < kQgWaves; w++) v += part[(w * NT + j) * kWave + lane];
    return v;
}

}  // namespace
}  // namespace l2z
