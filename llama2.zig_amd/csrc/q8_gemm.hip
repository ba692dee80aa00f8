// q8_gemm.hip -- the GEMM of the batched prompt pass on int8 group-quantized weights, on the int8
// matrix cores.  Compiled with -ffp-contract=off like every kernel file: every FMA here is an explicit one.
//
//   out[t][i] = sum over groups g of  f32(I[t][i][g]) * ws[i][g] * xs[t][g],   I = sum over the group of wq * xq   (int32, exact)
//
// The operand layout, the K loop and both summation orders are q8_gemm_device.h's, which the batched step's launches
// (q8_batch.hip) run too.  A lane ends with four consecutive output features of one token: a 16-byte store, and two
// W1 | W3 pairs of the interleaved slot, so SwiGLU is lane-local.
//
// A block of eight waves owns 16 weight rows and up to NT tiles of 16 tokens.  Which wave takes which group and both
// orders are functions of n and gs alone: the same bits from run to run, whatever the other rows of the call hold and
// however many there are.  No atomics.
#include "q8_gemm_device.h"

namespace l2z {
namespace {

template <int EPI, int GS, int NT>
__global__ __launch_bounds__(kQgBlock) void q8_gemm_kernel(const Q8GemmArgs a)
{
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
    q8_gemm_wave_sums<GS, NT>(ap, a_in, wsp, bp, xsp, n, nt, wave, acc);
    // the K ranges' sums of a tile, added in wave order by the wave that stores the tile
    q8_gemm_stash<NT>(part, acc, wave, lane);
    for (int j = wave; j < nt; j += kQgWaves) {
        v4f v = q8_gemm_tile_sum<NT>(part, j, lane);
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
