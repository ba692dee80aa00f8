// packed_w.hip -- builds the 29-bit packed copy of the decode mat-vec weights (packed_w.h) on the
// device, and decodes it back to f32 for the tests.  One pass over each f32 matrix for its exponent range, one to pack.
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

}  // namespace l2z
