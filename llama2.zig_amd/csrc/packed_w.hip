// packed_w.hip -- builds the 29-bit and 28-bit packed copies of the decode mat-vec weights (packed_w.h) on
// the device, and decodes them back to f32 for the tests.  One pass over each f32 matrix for its exponent range, one over
// a 28-bit candidate for its escapes, one to pack.
#include "kernel_common.h"
#include "packed_w.h"

namespace l2z {
namespace {

// stats[0] max biased exponent of the nonzero values, [1] min of them, [2] NaN / Inf / denormal seen
__global__ __launch_bounds__(256) void pk_stats_kernel(const uint32_t *__restrict__ p, size_t count, uint32_t *stats)
{
    uint32_t mx = 0, mn = 255, bad = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
        const uint32_t v = p[i], e = (v >> 23) & 0xffu;
        if (e == 255u || (e == 0u && (v & 0x7fffffu) != 0u)) bad = 1;
        if (e != 0u) {
            mx = e > mx ? e : mx;
            mn = e < mn ? e : mn;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t omx = __shfl_xor(mx, o, 64), omn = __shfl_xor(mn, o, 64), ob = __shfl_xor(bad, o, 64);
        mx = omx > mx ? omx : mx;
        mn = omn < mn ? omn : mn;
        bad |= ob;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMax(stats + 0, mx);
        atomicMin(stats + 1, mn);
        if (bad) atomicOr(stats + 2, 1u);
    }
}

// block (pair q, batch b), thread = the row kernel's lane tid: its values of rows 2q, 2q + 1 of the row-major matrix
// m (n4 float4 per row)
template <int S>
__device__ __forceinline__ void pk_pack_lane(const uint32_t *ra, const uint32_t *rb, int c4, int e_base, uint32_t *dst)
{
    uint32_t v[8 * S > 0 ? 8 * S : 1], d[pk::lane_dw(S) > 0 ? pk::lane_dw(S) : 1];
#pragma unroll
    for (int k = 0; k < S; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v[8 * k + j] = ra[4 * (c4 + 256 * k) + j];
            v[8 * k + 4 + j] = rb[4 * (c4 + 256 * k) + j];
        }
#pragma unroll
    for (int i = 0; i < pk::lane_dw(S); i++) d[i] = 0;
    pk::encode_lane<S>(v, e_base, d);
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < pk::lane_dw(S); i++) dst[pk::plane_off(S, i, lane)] = d[i];
}

template <int S>
__device__ __forceinline__ void pk_unpack_lane(const uint32_t *src, int c4, int e_base, uint32_t *oa, uint32_t *ob)
{
    const int lane = threadIdx.x & 63;
    constexpr int N = pk::lane_dw(S);
    uint32_t d[N > 0 ? N : 1], t[8 * S > 0 ? 8 * S : 1];
#pragma unroll
    for (int i = 0; i < N; i++) d[i] = src[pk::plane_off(S, i, lane)];
    pk::decode_lane_t<S>(d, t);
#pragma unroll
    for (int k = 0; k < S; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            oa[4 * (c4 + 256 * k) + j] = __float_as_uint(__builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + j]), e_base - 31));
            ob[4 * (c4 + 256 * k) + j] = __float_as_uint(__builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 4 + j]), e_base - 31));
        }
}

template <bool PACK>
__global__ __launch_bounds__(256) void pk_pack_kernel(const uint32_t *m, uint32_t *pk, uint32_t *out, int n, int e_base)
{
    const int n4 = n >> 2, q = blockIdx.x, b = blockIdx.y, w = threadIdx.x >> 6;
    const int s = pk::steps(n4, b, w);
    const size_t base = (size_t)q * pk::pair_dw(n4) + pk::chunk_off(n4, b, w);
    const int c4 = b * pk::kBatchF4 + threadIdx.x;
    const size_t ra = (size_t)(2 * q) * n, rb = ra + n;
    switch (s) {
#define L2Z_PK_CASE(S_)                                                            \
    case S_:                                                                       \
        if (PACK) pk_pack_lane<S_>(m + ra, m + rb, c4, e_base, pk + base);         \
        else pk_unpack_lane<S_>(pk + base, c4, e_base, out + ra, out + rb);        \
        break;
        L2Z_PK_CASE(1)
        L2Z_PK_CASE(2)
        L2Z_PK_CASE(3)
        L2Z_PK_CASE(4)
#undef L2Z_PK_CASE
        default: break;
    }
}


// ---- the 28-bit form (packed_w.h pk28): rows of exactly one batch, a block per pair ----

// the lane's 32 values of pair rows ra / rb in i order (the row kernel's lane tid of the pair's only batch)
__device__ __forceinline__ void pk28_lane_values(const uint32_t *ra, const uint32_t *rb, uint32_t (&v)[32])
{
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v[8 * k + j] = ra[4 * (threadIdx.x + 256 * k) + j];
            v[8 * k + 4 + j] = rb[4 * (threadIdx.x + 256 * k) + j];
        }
}

// max_esc: the most escapes any pair of the matrix has (preset 0)
__global__ __launch_bounds__(256) void pk28_count_kernel(const uint32_t *m, int e_base, uint32_t *max_esc)
{
    __shared__ uint32_t part[4];
    const uint32_t *pr = m + (size_t)blockIdx.x * (2 * 4096);
    uint32_t n = 0;
    for (int i = threadIdx.x; i < 2 * 4096; i += 256) n += pk28::is_escape(pr[i], e_base) ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = part[0] + part[1] + part[2] + part[3];
        if (t > 0) atomicMax(max_esc, t);
    }
}

// stream and patch record of pair blockIdx.x.  The record is compacted in pos order (thread order, then i): every thread
// finds its first entry from the counts of the threads before it, so no atomic decides the order
__global__ __launch_bounds__(256) void pk28_pack_kernel(const uint32_t *m, uint32_t *pk, uint32_t *rec, int e_base)
{
    __shared__ uint32_t cnt[256];
    __shared__ uint32_t r[pk28::kRecDw];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t *ra = m + (size_t)(2 * q) * 4096, *rb = ra + 4096;
    uint32_t v[32], d[pk28::kLaneDw];
    pk28_lane_values(ra, rb, v);
    const uint32_t esc = pk28::encode_lane(v, e_base, d);
    uint32_t *dst = pk + (size_t)q * pk28::kPairDw + w * pk28::kChunkDw;
#pragma unroll
    for (int i = 0; i < pk28::kLaneDw; i++) dst[pk28::plane_off(i, lane)] = d[i];
    cnt[tid] = __popc(esc);
    if (tid < pk28::kRecDw) r[tid] = (tid & 1) ? 0u : pk28::kNoEsc;
    __syncthreads();
    if (esc != 0u) {
        uint32_t at = 0;
        for (int t = 0; t < tid; t++) at += cnt[t];
#pragma unroll
        for (int i = 0; i < 32; i++)
            if ((esc >> i) & 1u) {
                if (at < (uint32_t)pk28::kMaxEsc) {
                    r[2 * at] = pk28::esc_pos(w, lane, i);
                    r[2 * at + 1] = v[i];
                }
                at++;
            }
    }
    __syncthreads();
    if (tid < pk28::kRecDw) rec[(size_t)q * pk28::kRecDw + tid] = r[tid];
}

__global__ __launch_bounds__(256) void pk28_unpack_kernel(const uint32_t *pk, const uint32_t *rec, uint32_t *out, int e_base)
{
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t *src = pk + (size_t)q * pk28::kPairDw + w * pk28::kChunkDw;
    uint32_t d[pk28::kLaneDw], t[32];
#pragma unroll
    for (int i = 0; i < pk28::kLaneDw; i++) d[i] = src[pk28::plane_off(i, lane)];
    pk28::decode_lane_t(d, t);
    uint32_t *oa = out + (size_t)(2 * q) * 4096, *ob = oa + 4096;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            oa[4 * (tid + 256 * k) + j] = __float_as_uint(__builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + j]), e_base - 15));
            ob[4 * (tid + 256 * k) + j] = __float_as_uint(__builtin_amdgcn_ldexpf(__uint_as_float(t[8 * k + 4 + j]), e_base - 15));
        }
    // the escapes this thread owns, over its own stores above
    for (int k = 0; k < pk28::kMaxEsc; k++) {
        const uint32_t pos = rec[(size_t)q * pk28::kRecDw + 2 * k];
        if (pos == pk28::kNoEsc || (pos >> 5) != (uint32_t)tid) continue;
        const int i = pos & 31u;
        ((i & 4) ? ob : oa)[4 * (tid + 256 * (i >> 3)) + (i & 3)] = rec[(size_t)q * pk28::kRecDw + 2 * k + 1];
    }
}

}  // namespace

hipError_t launch_pk_stats(const float *m, size_t count, uint32_t *stats, hipStream_t st)
{
    size_t blocks = (count + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(pk_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t *)m, count, stats);
    return hipGetLastError();
}

hipError_t launch_pk_pack(const float *m, int rows, int n, int e_base, uint32_t *pk, hipStream_t st)
{
    if (!pk::width_ok(n) || rows <= 0 || rows % 2) return hipErrorInvalidValue;
    const dim3 grid(rows / 2, (n / 4 + pk::kBatchF4 - 1) / pk::kBatchF4);
    hipLaunchKernelGGL(pk_pack_kernel<true>, grid, dim3(256), 0, st, (const uint32_t *)m, pk, nullptr, n, e_base);
    return hipGetLastError();
}

hipError_t launch_pk_unpack(const uint32_t *pk, int rows, int n, int e_base, float *out, hipStream_t st)
{
    if (!pk::width_ok(n) || rows <= 0 || rows % 2) return hipErrorInvalidValue;
    const dim3 grid(rows / 2, (n / 4 + pk::kBatchF4 - 1) / pk::kBatchF4);
    hipLaunchKernelGGL(pk_pack_kernel<false>, grid, dim3(256), 0, st, nullptr, const_cast<uint32_t *>(pk),
                       (uint32_t *)out, n, e_base);
    return hipGetLastError();
}

hipError_t launch_pk28_count(const float *m, int rows, int n, int e_base, uint32_t *max_esc, hipStream_t st)
{
    if (!pk28::width_ok(n) || rows <= 0 || rows % 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pk28_count_kernel, dim3(rows / 2), dim3(256), 0, st, (const uint32_t *)m, e_base, max_esc);
    return hipGetLastError();
}

hipError_t launch_pk28_pack(const float *m, int rows, int n, int e_base, uint32_t *pk, uint32_t *rec, hipStream_t st)
{
    if (!pk28::width_ok(n) || rows <= 0 || rows % 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pk28_pack_kernel, dim3(rows / 2), dim3(256), 0, st, (const uint32_t *)m, pk, rec, e_base);
    return hipGetLastError();
}

hipError_t launch_pk28_unpack(const uint32_t *pk, const uint32_t *rec, int rows, int n, int e_base, float *out, hipStream_t st)
{
    if (!pk28::width_ok(n) || rows <= 0 || rows % 2) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pk28_unpack_kernel, dim3(rows / 2), dim3(256), 0, st, pk, rec, (uint32_t *)out, e_base);
    return hipGetLastError();
}

}  // namespace l2z
