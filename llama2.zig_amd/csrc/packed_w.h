// packed_w.h -- the lossless 29-bit form of the decode mat-vec weights: the format, shared by the
// kernel that builds it (packed_w.hip), the row kernel that streams it (matvec.hip) and the test read-back.
//
// Per matrix a base E = the largest biased exponent of its values.  A value of biased exponent e in [E - 30, E] gets the
// 5-bit code c = e - (E - 31) in 1..31, +-0 gets c = 0; T = sign | c << 23 | mantissa is then a float whose value times
// 2^(E - 31) is exactly the original (ldexp: the result is normal, or +-0 from c = 0).  A matrix with a NaN, an Inf, a
// denormal or a value below that window stays f32 (encodable()).
//
// Layout, in the row kernel's own consumption order (matvec_row_kernel: a block owns a pair of rows, lane `tid` of a
// batch b takes float4 columns b * 1024 + tid + 256 k of both rows, k < 4; a wave's steps past the row end load
// nothing).  One lane's values of one batch, i = 8 k + 4 r + j (step k, row r of the pair, component j), S in-row
// steps, 8 S values in lane_dw(S) = ceil(29 S / 4) dwords (S = 4: 32 values, 29 dwords, 116 bytes):
//   dword d < lane_dw(S) holds T(value d) in bits 31, 27..0; its bits 28..30 carry 3 bits of a stream that holds the
//   remaining X = 8 S - lane_dw(S) values (0..3) as 29-bit words P = rotl(T, 1) (bit b of the stream: bit 28 + b % 3
//   of dword b / 3).
// A wave's dwords of one batch are [lane_dw / 4 planes of 16 bytes per lane][lane_dw % 4 planes of 4 bytes per lane],
// each plane lane-major: every load instruction is a linear sweep of 64 x 16 or 64 x 4 bytes.  A pair's chunks follow in
// (batch, wave) order, pairs in row order: pair q of a matrix starts at q * pair_dw(n / 4).
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace l2z {
namespace pk {

constexpr int kMaxLaneDw = 29;
constexpr int kBatchF4 = 1024;  // float4 columns per batch of a row (256 lanes x 4 steps)

__host__ __device__ constexpr int lane_dw(int s) { return (29 * s + 3) / 4; }
// dword i of a lane's chunk: its offset in the wave's chunk of lane_dw(s) * 64 dwords
__host__ __device__ constexpr int plane_off(int s, int i, int lane)
{
    return i < lane_dw(s) / 4 * 4 ? (i / 4) * 256 + lane * 4 + i % 4 : lane_dw(s) / 4 * 256 + (i - lane_dw(s) / 4 * 4) * 64 + lane;
}

// in-row steps of wave w in batch b of a row of n4 float4 (the fp32 kernel's `in_row`, wave-uniform)
__host__ __device__ inline int steps(int n4, int b, int w)
{
    int s = 0;
    for (int k = 0; k < 4; k++) s += (b * kBatchF4 + 64 * w + 256 * k < n4) ? 1 : 0;
    return s;
}

// dword offset of wave w's chunk of batch b inside its pair
__host__ __device__ inline size_t chunk_off(int n4, int b, int w)
{
    size_t o = (size_t)b * 4 * 64 * kMaxLaneDw;  // every batch but the last is full
    for (int v = 0; v < w; v++) o += (size_t)64 * lane_dw(steps(n4, b, v));
    return o;
}

__host__ __device__ inline size_t pair_dw(int n4)
{
    const int nb = (n4 + kBatchF4 - 1) / kBatchF4;
    return chunk_off(n4, nb - 1, 4);
}

// a row width the packed row kernel takes (the fp32 row kernel's: n4 >= 1024, n4 % 64 == 0)
__host__ __device__ constexpr bool width_ok(int n) { return n % 256 == 0 && n >= 4096; }

__host__ __device__ inline uint32_t encode_t(uint32_t v, int e_base)
{
    const uint32_t e = (v >> 23) & 0xffu;
    const uint32_t c = e == 0 ? 0u : e - (uint32_t)(e_base - 31);
    return (v & 0x807fffffu) | (c << 23);
}

// the stats of one matrix (stats kernel): largest and smallest biased exponent of the nonzero values, and whether any
// value is a NaN, an Inf or a denormal
__host__ __device__ inline bool encodable(uint32_t max_e, uint32_t min_e, uint32_t bad)
{
    return bad == 0 && (max_e == 0 || min_e + 30 >= max_e);
}

// v: the lane's 8 S values (bits) in i order -> d: lane_dw(S) dwords
template <int S>
__host__ __device__ inline void encode_lane(const uint32_t *v, int e_base, uint32_t *d)
{
    constexpr int N = lane_dw(S), X = 8 * S - N;
#pragma unroll
    for (int i = 0; i < N; i++) d[i] = encode_t(v[i], e_base);
#pragma unroll
    for (int x = 0; x < X; x++) {
        const uint32_t t = encode_t(v[N + x], e_base);
        const uint32_t p = ((t << 1) | (t >> 31)) & 0x1fffffffu;
#pragma unroll
        for (int b = 0; b < 29; b++) {
            const int s = 29 * x + b;
            d[s / 3] |= ((p >> b) & 1u) << (28 + s % 3);
        }
    }
}

// d: lane_dw(S) dwords -> T words of the 8 S values (value = ldexp(T as float, E - 31))
template <int S>
__host__ __device__ inline void decode_lane_t(const uint32_t *d, uint32_t *t)
{
    constexpr int N = lane_dw(S), X = 8 * S - N;
#pragma unroll
    for (int i = 0; i < N; i++) t[i] = d[i] & 0x8fffffffu;
#pragma unroll
    for (int x = 0; x < X; x++) {
        uint32_t p = 0;
#pragma unroll
        for (int q = (29 * x) / 3; q <= (29 * x + 28) / 3; q++) {  // dwords holding stream bits [29x, 29x + 29)
            const int lo = 29 * x > 3 * q ? 29 * x : 3 * q;
            const int hi = 29 * x + 29 < 3 * q + 3 ? 29 * x + 29 : 3 * q + 3;
            const uint32_t piece = (d[q] >> (28 + lo - 3 * q)) & ((1u << (hi - lo)) - 1u);
            p |= piece << (lo - 29 * x);
        }
        t[N + x] = (p >> 1) | (p << 31);
    }
}

}  // namespace pk
}  // namespace l2z
