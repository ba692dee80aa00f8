// q8_batch.hip -- the two launches of its own the batched step has on int8 group-quantized weights (host
// side: batch_host.cpp batch_step_q8): q | k | v of a layer in ONE launch, with RoPE at each row's own position and K / V
// stored straight into the row's own caches, and the classifier with each row's logits stored through the step's table.
// Wo, W1 | W3 and W2 of the step are q8_gemm.hip's launches as they stand.  Compiled with -ffp-contract=off like every
// kernel file.
//
// The products are q8_gemm_device.h's body at ONE token tile (a step has at most 16 rows): the bits of a row's product are
// the bits q8_gemm_kernel gives for the same quantized row and matrix, whatever the other rows of the tile hold.  The
// quantized rows stand padded to the tile (q8_rows.hip writes rows m .. 15 as zeros); a pad row has NO table entry: the
// epilogues neither read the table for it nor store anything.  Wave 0 stores the tile: a lane holds four consecutive
// features of one row -- two RoPE pairs of one head (head_size % 4 == 0), one 16-byte store.  No atomics.
#include "batch_decode.h"
#include "q8_gemm_device.h"
#include "rope_device.h"

namespace l2z {
namespace {

// what the two kernels share: this lane's operands of row tile `tile` of a [d, n] matrix -> its four sums of token row
// `lane & 15`, valid in wave 0 after the call.  *o_row: the first of the lane's four output rows; false: they lie past the
// matrix (d is a multiple of 4: all four or none)
template <int GS>
__device__ __forceinline__ bool q8_batch_tile(const int8_t *wq, const float *ws, const int8_t *xq, const float *xs, int n,
                                              int d, int tile, v4f *part, v4f *sum, int *o_row)
{
    constexpr int LB = GS / 4;  // bytes of a group a lane holds
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int ng = n / GS, row0 = tile * 16;
    const int a_row = row0 + col;
    *o_row = row0 + 4 * quad;
    const bool a_in = a_row < d, o_in = *o_row < d;
    const int8_t *ap = wq + (size_t)(a_in ? a_row : 0) * (size_t)n + quad * LB;
    const float *wsp = ws + (size_t)(o_in ? *o_row : 0) * (size_t)ng;
    const int8_t *bp = xq + (size_t)col * (size_t)n + quad * LB;
    const float *xsp = xs + (size_t)col * (size_t)ng;
    v4f acc[1];
    q8_gemm_wave_sums<GS, 1>(ap, a_in, wsp, bp, xsp, n, 1, wave, acc);
    q8_gemm_stash<1>(part, acc, wave, lane);
    if (wave != 0) return false;
    *sum = q8_gemm_tile_sum<1>(part, 0, lane);
    return o_in;
}

// Block b is (segment, row tile): the tq tiles of Wq first, then the tkv of Wk, then those of Wv -- three allocations, each
// with its own tile count and its own last tile that need not be full (dim or kv_dim no multiple of 16).
template <int GS>
__global__ __launch_bounds__(kQgBlock) void q8_batch_qkv_kernel(const Q8BatchQkvArgs a)
{
    __shared__ v4f part[kQgWaves * kWave];
    const int tq = (a.dim + 15) / 16, tkv = (a.kvd + 15) / 16;
    const int b = blockIdx.x;
    const int seg = b < tq ? 0 : b < tq + tkv ? 1 : 2;   // (block-uniform)
    const int tile = seg == 0 ? b : seg == 1 ? b - tq : b - tq - tkv;
    const int8_t *wq = seg == 0 ? a.wq_q : seg == 1 ? a.wq_k : a.wq_v;
    const float *ws = seg == 0 ? a.ws_q : seg == 1 ? a.ws_k : a.ws_v;
    v4f v;
    int f;
    if (!q8_batch_tile<GS>(wq, ws, a.xq, a.xs, a.n, seg == 0 ? a.dim : a.kvd, tile, part, &v, &f)) return;
    const int row = threadIdx.x & 15;
    if (row >= a.m) return;   // a pad row: no table entry
    const int pos = a.tab->pos[row];
    if (seg != 2) v = rope_rotate4(v, rope_cs4(a.rope, pos, a.hs, f));   // main.zig:336-351
    if (seg == 0) {
        *(v4f *)(a.q + (size_t)row * (size_t)a.ldq + f) = v;
        return;
    }
    // head-major cache [kv head][seq_len][head_size]: the row's own, at its own position (:354-358)
    float *cache = (seg == 1 ? a.tab->kc[row] : a.tab->vc[row]) + a.layer_off;
    *(v4f *)(cache + (size_t)(f / a.hs) * a.kv_head_stride + (size_t)pos * (size_t)a.hs + (size_t)(f % a.hs)) = v;
}

// main.zig:429 for the rows of a step: row r's logits through tab->logits[r]
template <int GS>
__global__ __launch_bounds__(kQgBlock) void q8_batch_cls_kernel(const Q8BatchClsArgs a)
{
    __shared__ v4f part[kQgWaves * kWave];
    v4f v;
    int f;
    if (!q8_batch_tile<GS>(a.wq, a.ws, a.xq, a.xs, a.n, a.vocab, blockIdx.x, part, &v, &f)) return;
    const int row = threadIdx.x & 15;
    if (row >= a.m) return;   // a pad row: no table entry
    *(v4f *)(a.tab->logits[row] + f) = v;
}

bool q8_batch_operands_ok(const int8_t *xq, const float *xs, int m, int n, int gs)
{
    return (gs == 32 || gs == 64) && m >= 1 && m <= kBatchMax && n > 0 && n % gs == 0 && xq != nullptr && xs != nullptr &&
           aligned16(xq);
}

}  // namespace

hipError_t launch_q8_batch_qkv(const Q8BatchQkvArgs &a, hipStream_t st)
{
    if (!q8_batch_operands_ok(a.xq, a.xs, a.m, a.n, a.gs) || a.tab == nullptr || a.rope == nullptr || a.q == nullptr)
        return hipErrorInvalidValue;
    if (a.wq_q == nullptr || a.wq_k == nullptr || a.wq_v == nullptr || a.ws_q == nullptr || a.ws_k == nullptr || a.ws_v == nullptr ||
        !aligned16(a.wq_q) || !aligned16(a.wq_k) || !aligned16(a.wq_v))
        return hipErrorInvalidValue;
    // a lane's four features are two RoPE pairs of one head and one 16-byte store into q or a cache row
    if (a.hs <= 0 || (a.hs & 3) != 0 || a.dim <= 0 || a.kvd <= 0 || a.dim % a.hs != 0 || a.kvd % a.hs != 0 || (a.ldq & 3) != 0 ||
        a.ldq < a.dim || !aligned16(a.q) || !aligned16(a.rope) || (a.layer_off & 3) != 0 || (a.kv_head_stride & 3) != 0)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a.dim + 15) / 16 + 2 * ((a.kvd + 15) / 16));
    if (a.gs == 32)
        hipLaunchKernelGGL(q8_batch_qkv_kernel<32>, dim3(blocks), dim3(kQgBlock), 0, st, a);
    else
        hipLaunchKernelGGL(q8_batch_qkv_kernel<64>, dim3(blocks), dim3(kQgBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_q8_batch_cls(const Q8BatchClsArgs &a, hipStream_t st)
{
    if (!q8_batch_operands_ok(a.xq, a.xs, a.m, a.n, a.gs) || a.tab == nullptr || a.wq == nullptr || a.ws == nullptr ||
        !aligned16(a.wq) || a.vocab <= 0 || (a.vocab & 3) != 0)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((a.vocab + 15) / 16);
    if (a.gs == 32)
        hipLaunchKernelGGL(q8_batch_cls_kernel<32>, dim3(blocks), dim3(kQgBlock), 0, st, a);
    else
        hipLaunchKernelGGL(q8_batch_cls_kernel<64>, dim3(blocks), dim3(kQgBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace l2z
