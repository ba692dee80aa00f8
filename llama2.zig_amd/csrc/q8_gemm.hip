// q8_gemm.hip -- the GEMM of the batched prompt pass on int8 group-quantized weights, on the int8
// matrix cores.  Compiled with -ffp-contract=off like every kernel file: every FMA here is an explicit one.
//
//   out[t][i] = sum over groups g of  f32(I[t][i][g]) * ws[i][g] * xs[t][g],   I = sum over the group of wq * xq   (int32, exact)
//
// Both operands are K-contiguous int8 rows, so a lane's MFMA operand is one load from either matrix: the weight rows are
// the A side (the tile's 16 rows), the token rows the B side (its 16 columns).  One MFMA into a zeroed tile is exactly one
// group's I for 16 x 16 (row, token) pairs -- v_mfma_i32_16x16x64_i8 at group size 64 (16 bytes a lane from either
// matrix), v_mfma_i32_16x16x32_i8 at 32 (8 bytes) --, so a group never shares an MFMA with another and K is any whole
// number of groups (dim 288 at group size 32: nine).  A and B of a lane cover the same 16 (8) values of the group, so the
// tile is the sum over the whole group whatever order the instruction takes them in.  The result tile has the token on
// the lane (lane & 15) and four consecutive weight rows in its registers (4 (lane >> 4) + r): after each group the four
// int32 are converted, scaled by their rows' ws[g] and the token's xs[g] -- (f32(I) * ws) * xs, the decode's order, the
// second product fused into the sum -- and added to the lane's four f32 sums.  Four consecutive output features of one
// token a lane: a 16-byte store, and two W1 | W3 pairs of the interleaved slot, so SwiGLU is lane-local.
//
// A block of eight waves owns 16 weight rows and up to NT tiles of 16 tokens.  The waves split K: wave w takes groups w,
// w + 8, ... in increasing order (together the eight read 512 (256) contiguous bytes of each of the 16 rows per step),
// leaves its partial sums in LDS, and the sums of a tile are then added in wave order 0 .. 7 by the wave that stores
// it.  Which wave takes which group and both orders are functions of n and gs alone: the same bits from run to run,
// whatever the other rows of the call hold and however many there are.  No atomics.
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

template <int EPI, int GS, int NT>
__global__ __launch_bounds__(kQgBlock) void q8_gemm_kernel(const Q8GemmArgs a)
{
    typedef typename Q8Frag<GS>::T Frag;
    constexpr int LB = GS / 4;  // bytes of a group a lane holds
    __shared__ v4f part[kQgWaves * NT * kWave];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int n = a.n, ng = n / GS;
    const int n_tiles = (a.m + kQ8GemmTile - 1) / kQ8GemmTile, n_tt = (n_tiles + NT - 1) / NT;
    const int tile0 = (blockIdx.x % n_tt) * NT, row0 = (blockIdx.x / n_tt) * 16;
    const int nt = n_tiles - tile0 < NT ? n_tiles - tile0 : NT;  // token tiles of this block (block-uniform)
    // A: weight row row0 + col (past the matrix: zeros); its four output rows' scales: rows row0 + 4 quad + r, all in the
    // matrix or none (d is a multiple of 4)
    const int a_row = row0 + col, o_row = row0 + 4 * quad;
    const bool a_in = a_row < a.d, o_in = o_row < a.d;
    const int8_t *ap = a.wq + (size_t)(a_in ? a_row : 0) * (size_t)n + quad * LB;
    const float *wsp = a.ws + (size_t)(o_in ? o_row : 0) * (size_t)ng;
    // B: token row 16 (tile0 + j) + col (the rows stand padded to whole tiles), and its scales
    const int8_t *bp = a.xq + (size_t)(tile0 * kQ8GemmTile + col) * (size_t)n + quad * LB;
    const float *xsp = a.xs + (size_t)(tile0 * kQ8GemmTile + col) * (size_t)ng;

    v4f acc[NT];
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
    // the K ranges' sums of a tile, added in wave order by the wave that stores the tile
#pragma unroll
    for (int j = 0; j < NT; j++) part[(wave * NT + j) * kWave + lane] = acc[j];
    __syncthreads();
    for (int j = wave; j < nt; j += kQgWaves) {
        v4f v = part[j * kWave + lane];
#pragma unroll
        for (int w = 1; w < kQgWaves; w++) v += part[(w * NT + j) * kWave + lane];
        const int t = (tile0 + j) * kQ8GemmTile + col;
        if (t >= a.m || !o_in) continue;
        if (EPI == EPI_SWIGLU) {  // rows 2p, 2p + 1 = W1 row p, W3 row p: two gated values (main.zig:411-416)
            v2f h;
            h.x = v.x * (1.0f / (1.0f + expf(-v.x)));
            h.x = h.x * v.y;
            h.y = v.z * (1.0f / (1.0f + expf(-v.z)));
            h.y = h.y * v.w;
            *(v2f *)(a.out + (size_t)t * (size_t)a.ldo + (o_row >> 1)) = h;
        } else {
            if (EPI == EPI_RESID) v = *(const v4f *)(a.res + (size_t)t * (size_t)a.ldres + o_row) + v;  // :395 / :422
            *(v4f *)(a.out + (size_t)t * (size_t)a.ldo + o_row) = v;
        }
    }
}

template <int GS, int NT>
const void *q8_gemm_pick(int epi)
{
    switch (epi) {
        case EPI_STORE: return reinterpret_cast<const void *>(&q8_gemm_kernel<EPI_STORE, GS, NT>);
        case EPI_RESID: return reinterpret_cast<const void *>(&q8_gemm_kernel<EPI_RESID, GS, NT>);
        case EPI_SWIGLU: return reinterpret_cast<const void *>(&q8_gemm_kernel<EPI_SWIGLU, GS, NT>);
        default: return nullptr;
    }
}

template <int GS>
const void *q8_gemm_pick_nt(int epi, int nt)
{
    switch (nt) {
        case 1: return q8_gemm_pick<GS, 1>(epi);
        case 2: return q8_gemm_pick<GS, 2>(epi);
        case 4: return q8_gemm_pick<GS, 4>(epi);
        default: return q8_gemm_pick<GS, 8>(epi);
    }
}

}  // namespace

hipError_t launch_q8_gemm(const Q8GemmArgs &a, int epi, hipStream_t st)
{
    if ((a.gs != 32 && a.gs != 64) || a.m <= 0 || a.n <= 0 || a.n % a.gs != 0 || a.d <= 0 || (a.d & 3) != 0) return hipErrorInvalidValue;
    if (a.xq == nullptr || a.xs == nullptr || a.wq == nullptr || a.ws == nullptr || a.out == nullptr) return hipErrorInvalidValue;
    // 16-byte loads of both operands' rows (n is a multiple of 32), 16-byte stores of four features (SwiGLU: 8 of two)
    if (!aligned16(a.xq) || !aligned16(a.wq) || !aligned16(a.out) || (a.ldo & 3) != 0 || a.ldo < (epi == EPI_SWIGLU ? a.d / 2 : a.d))
        return hipErrorInvalidValue;
    if (epi == EPI_RESID && (a.res == nullptr || !aligned16(a.res) || (a.ldres & 3) != 0 || a.ldres < a.d)) return hipErrorInvalidValue;
    // token tiles a block: all of a short chunk's, at most 8 (the weights' 16 rows are read once per block)
    const int n_tiles = (a.m + kQ8GemmTile - 1) / kQ8GemmTile;
    const int nt = n_tiles <= 1 ? 1 : n_tiles <= 2 ? 2 : n_tiles <= 4 ? 4 : 8;
    const void *fn = a.gs == 32 ? q8_gemm_pick_nt<32>(epi, nt) : q8_gemm_pick_nt<64>(epi, nt);
    if (fn == nullptr) return hipErrorInvalidValue;
    const long long blocks = (long long)((a.d + 15) / 16) * ((n_tiles + nt - 1) / nt);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    Q8GemmArgs args = a;
    void *params[] = {&args};
    return hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(kQgBlock), params, 0, st);
}

}  // namespace l2z
