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

// The 28-bit form: the same scheme with a 4-bit exponent code, for slots whose rows are exactly one full
// batch wide (n == 4096: every lane holds 32 values).  A value of biased exponent e in [E - 14, E] gets the code
// c = e - (E - 15) in 1..15, +-0 gets c = 0, T = sign | c << 23 | mantissa and ldexp(T, E - 15) is the original.  A nonzero
// value BELOW that window (e in [E - 30, E - 15]: encodable() still bounds the span) is an ESCAPE: the stream holds +0 in
// its place and its f32 bits stand in the pair's patch record.  A slot in which any pair has more than kMaxEsc escapes
// keeps the 29-bit form.
//
// Lane layout: 32 values i = 8 k + 4 r + j in 28 dwords.  Dword d < 28 holds T(value d) in bits 31 and 26..0; its bits
// 27..30 carry 4 bits of a stream that holds values 28..31 as 28-bit words P = rotl(T, 1) (bit b of the stream: bit
// 27 + b % 4 of dword b / 4, so value 28 + x is the seven nibbles of dwords 7 x .. 7 x + 6).  A wave's chunk is 7 planes
// of 16 bytes per lane, lane-major (7168 bytes); a pair is its 4 waves' chunks (28672 bytes), pairs in row order.
//
// Patch record of a pair: 16 dwords, kMaxEsc entries {pos, bits} sorted by pos = wave << 11 | lane << 5 | i; the unused
// entries come last with pos = kNoEsc (and bits 0).
namespace pk28 {

constexpr int kLaneDw = 28;
constexpr int kChunkDw = 64 * kLaneDw;   // one wave
constexpr int kPairDw = 4 * kChunkDw;    // 28672 bytes
constexpr int kMaxEsc = 8;
constexpr int kRecDw = 2 * kMaxEsc;      // 64 bytes
constexpr uint32_t kNoEsc = 0xffffffffu;

__host__ __device__ constexpr bool width_ok(int n) { return n == 4 * pk::kBatchF4; }
// dword i of a lane's chunk: its offset in the wave's chunk
__host__ __device__ constexpr int plane_off(int i, int lane) { return (i / 4) * 256 + lane * 4 + i % 4; }
__host__ __device__ constexpr uint32_t esc_pos(int wave, int lane, int i) { return (uint32_t)(wave << 11 | lane << 5 | i); }

__host__ __device__ inline bool is_escape(uint32_t v, int e_base)
{
    const int e = (int)((v >> 23) & 0xffu);
    return e != 0 && e < e_base - 14;
}

__host__ __device__ inline uint32_t encode_t(uint32_t v, int e_base)
{
    const uint32_t e = (v >> 23) & 0xffu;
    if (is_escape(v, e_base)) return 0u;
    const uint32_t c = e == 0 ? 0u : e - (uint32_t)(e_base - 15);
    return (v & 0x807fffffu) | (c << 23);
}

// v: the lane's 32 values (bits) in i order -> d: 28 dwords; returns the mask of the escapes among them (bit i)
__host__ __device__ inline uint32_t encode_lane(const uint32_t *v, int e_base, uint32_t *d)
{
    uint32_t esc = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) esc |= (is_escape(v[i], e_base) ? 1u : 0u) << i;
#pragma unroll
    for (int i = 0; i < kLaneDw; i++) d[i] = encode_t(v[i], e_base);
#pragma unroll
    for (int x = 0; x < 4; x++) {
        const uint32_t t = encode_t(v[kLaneDw + x], e_base);
        const uint32_t p = ((t << 1) | (t >> 31)) & 0x0fffffffu;
#pragma unroll
        for (int q = 0; q < 7; q++) d[7 * x + q] |= ((p >> (4 * q)) & 0xfu) << 27;
    }
    return esc;
}

// d: 28 dwords -> T words of the 32 values (value = ldexp(T as float, E - 15); an escape's T is +0)
__host__ __device__ inline void decode_lane_t(const uint32_t *d, uint32_t *t)
{
#pragma unroll
    for (int i = 0; i < kLaneDw; i++) t[i] = d[i] & 0x87ffffffu;
#pragma unroll
    for (int x = 0; x < 4; x++) {
        uint32_t p = 0;
#pragma unroll
        for (int q = 0; q < 7; q++) p |= ((d[7 * x + q] >> 27) & 0xfu) << (4 * q);
        t[kLaneDw + x] = (p >> 1) | (p << 31);
    }
}

// T -> the value's bits, what ldexp(T, E - 15) gives: the code back to the exponent, +-0 stays
__host__ __device__ inline uint32_t value_of_t(uint32_t t, int e_base)
{
    const uint32_t c = (t >> 23) & 0xffu;
    return c == 0 ? (t & 0x80000000u) : ((t & 0x807fffffu) | ((c + (uint32_t)(e_base - 15)) << 23));
}

__host__ __device__ inline void record_clear(uint32_t *rec)
{
    for (int k = 0; k < kMaxEsc; k++) {
        rec[2 * k] = kNoEsc;
        rec[2 * k + 1] = 0u;
    }
}

// One pair on the host (the statement the device packer is tested against): ra / rb the pair's two rows of 4096 values
// (bits) -> stream (kPairDw dwords) and rec (kRecDw dwords).  Returns the pair's number of escapes; more than kMaxEsc =
// overflow, the record then holds the first kMaxEsc in pos order.
inline int encode_pair(const uint32_t *ra, const uint32_t *rb, int e_base, uint32_t *stream, uint32_t *rec)
{
    int n_esc = 0;
    record_clear(rec);
    for (int w = 0; w < 4; w++)
        for (int lane = 0; lane < 64; lane++) {
            uint32_t v[32], d[kLaneDw];
            for (int k = 0; k < 4; k++)
                for (int j = 0; j < 4; j++) {
                    const int col = 4 * (64 * w + lane + 256 * k) + j;
                    v[8 * k + j] = ra[col];
                    v[8 * k + 4 + j] = rb[col];
                }
            const uint32_t esc = encode_lane(v, e_base, d);
            for (int i = 0; i < kLaneDw; i++) stream[w * kChunkDw + plane_off(i, lane)] = d[i];
            for (int i = 0; i < 32; i++)
                if ((esc >> i) & 1u) {
                    if (n_esc < kMaxEsc) {
                        rec[2 * n_esc] = esc_pos(w, lane, i);
                        rec[2 * n_esc + 1] = v[i];
                    }
                    n_esc++;
                }
        }
    return n_esc;
}

// ... and back: the pair's two rows' bits from stream and record
inline void decode_pair(const uint32_t *stream, const uint32_t *rec, int e_base, uint32_t *ra, uint32_t *rb)
{
    for (int w = 0; w < 4; w++)
        for (int lane = 0; lane < 64; lane++) {
            uint32_t d[kLaneDw], t[32];
            for (int i = 0; i < kLaneDw; i++) d[i] = stream[w * kChunkDw + plane_off(i, lane)];
            decode_lane_t(d, t);
            for (int i = 0; i < 32; i++) t[i] = value_of_t(t[i], e_base);
            for (int k = 0; k < kMaxEsc; k++)
                if (rec[2 * k] != kNoEsc && (rec[2 * k] >> 5) == (uint32_t)(64 * w + lane)) t[rec[2 * k] & 31u] = rec[2 * k + 1];
            for (int k = 0; k < 4; k++)
                for (int j = 0; j < 4; j++) {
                    const int col = 4 * (64 * w + lane + 256 * k) + j;
                    ra[col] = t[8 * k + j];
                    rb[col] = t[8 * k + 4 + j];
                }
        }
}

}  // namespace pk28
}  // namespace l2z
