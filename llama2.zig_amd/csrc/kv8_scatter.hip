// kv8_scatter.hip -- the write side of the int8 KV cache (kv8.h, kv8_layout.h): the launch that stands
// where launch_ragged_rope_scatter stands when the chunk's runstates hold int8 rows, and the conversion of f32 cache rows
// behind l2z_runstate_fork.  Both turn a slice into bytes and a scale through kv8_quant_slice (kv8_device.h) and nothing
// else.
//
// How the work is split.  A K or V slice of head_size values stands in TPR = kv8_lanes(head_size) consecutive lanes, a
// float4 a lane (the first head_size / 4 of them; 12 of 16 at head_size 48), so a block of 256 threads takes 256 / TPR
// slices a round and a slice never leaves a wave.  A round's trip count is uniform over the block: every lane of a group
// reaches the cross-lane maximum.  A lane reads its float4 once, rotates it (K), takes part in the maximum, quantizes its
// four values and stores them as ONE dword; lane 0 of the group stores the scale.  Vector loads and stores only; no fused
// multiply-add in the rotation (rope_device.h, -ffp-contract=off).
#include "kv8.h"

#include "kernel_common.h"
#include "kv8_device.h"
#include "rope_device.h"

namespace l2z {
namespace {

constexpr int kKv8Block = 256;

struct Kv8ScatterArgs {
    float *q;
    const float *k, *v;       // the chunk's key / value rows [P, kvd]
    const RaggedSeq *seq;     // (read for nothing: the slots' f32 pointers are null)
    const Kv8Seq *seq8;
    const int *row_seq, *row_pos;
    const float2 *rope;
    size_t layer_off, kv_head_stride;   // in values
    int ldq, dim, kvd, hs, seq_len;
};

// Block (row, y).  The q float4s of the row, rotated in place by the f32 scatter's statements; then the row's 2 * kv heads
// slices, K first.
__global__ __launch_bounds__(kKv8Block) void kv8_rope_scatter(const Kv8ScatterArgs a)
{
    const int row = blockIdx.x, tid = threadIdx.x, hs = a.hs;
    const int pos = a.row_pos[row];
    for (int i = blockIdx.y * kKv8Block + tid; i < (a.dim >> 2); i += gridDim.y * kKv8Block) {
        float *p = a.q + (size_t)row * a.ldq + 4 * i;
        const v4f x = *(const v4f *)p;
        *(v4f *)p = rope_rotate4(x, rope_cs4(a.rope, pos, hs, 4 * i));
    }
    const Kv8Seq sq = a.seq8[a.row_seq[row]];
    const int E = hs >> 2, TPR = kv8_lanes(hs), G = kKv8Block / TPR;
    const int kvh_n = a.kvd / hs, units = 2 * kvh_n;
    const int g = tid / TPR, c = tid % TPR;
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    for (int u0 = blockIdx.y * G; u0 < units; u0 += gridDim.y * G) {   // (uniform: every lane of a group takes the maximum)
        const int u = u0 + g;
        const bool live = u < units && c < E;
        const bool is_k = u < kvh_n;
        const int kvh = is_k ? u : u - kvh_n;
        v4f x = zero;
        if (live) {
            x = *(const v4f *)((is_k ? a.k : a.v) + (size_t)row * a.kvd + (size_t)kvh * hs + 4 * c);
            if (is_k) x = rope_rotate4(x, rope_cs4(a.rope, pos, hs, 4 * c));
        }
        float s;
        const int w = kv8_quant_slice(x, TPR, &s);
        if (live) {
            // head-major [kv head][seq_len][head_size] (kv8_layout.h); the scales: the same place less the innermost dimension
            const size_t at = a.layer_off + (size_t)kvh * a.kv_head_stride + (size_t)pos * (size_t)hs;
            *(int *)((is_k ? sq.k8 : sq.v8) + at + 4 * c) = w;
            if (c == 0) (is_k ? sq.ks : sq.vs)[at / (size_t)hs] = s;
        }
    }
}

// Block = 256 / TPR slices of rows 0 .. n_pos - 1 of the runs of an f32 cache, slice u = (run u / n_pos, row u % n_pos)
__global__ __launch_bounds__(kKv8Block) void kv8_quantize_cache(const float *src, int8_t *dst, float *dst_s, size_t units, int seq_len,
                                                                int hs, int n_pos)
{
    const int tid = threadIdx.x, E = hs >> 2, TPR = kv8_lanes(hs), G = kKv8Block / TPR;
    const int g = tid / TPR, c = tid % TPR;
    const size_t u = (size_t)blockIdx.x * G + g;
    const bool live = u < units && c < E;
    const size_t slice = live ? (u / (size_t)n_pos) * (size_t)seq_len + u % (size_t)n_pos : 0;
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    const v4f x = live ? *(const v4f *)(src + slice * (size_t)hs + 4 * c) : zero;
    float s;
    const int w = kv8_quant_slice(x, TPR, &s);
    if (live) {
        *(int *)(dst + slice * (size_t)hs + 4 * c) = w;
        if (c == 0) dst_s[slice] = s;
    }
}

}  // namespace

hipError_t launch_kv8_rope_scatter(float *q, int ldq, const RaggedChunk &rg, const Kv8Seq *seq8, int P, int dim, int kv_dim,
                                   int head_size, int seq_len, const float2 *rope, size_t layer_off, size_t kv_head_stride,
                                   hipStream_t st)
{
    if (P <= 0 || head_size < 4 || head_size > 256 || (head_size & 3) || (dim % head_size) || (kv_dim % head_size) || (ldq & 3) ||
        (((uintptr_t)q | (uintptr_t)rg.k | (uintptr_t)rg.v | (uintptr_t)rope) & 15) || (layer_off & 3) || (kv_head_stride & 3) ||
        seq8 == nullptr || rg.page_floats != 0 || seq_len < 1 || kv_head_stride != (size_t)seq_len * head_size)
        return hipErrorInvalidValue;
    Kv8ScatterArgs a = {};
    a.q = q; a.k = rg.k; a.v = rg.v; a.seq = rg.seq; a.seq8 = seq8; a.row_seq = rg.row_seq; a.row_pos = rg.row_pos; a.rope = rope;
    a.layer_off = layer_off; a.kv_head_stride = kv_head_stride;
    a.ldq = ldq; a.dim = dim; a.kvd = kv_dim; a.hs = head_size; a.seq_len = seq_len;
    const int lanes = (dim >> 2) + 2 * (kv_dim / head_size) * kv8_lanes(head_size);
    const dim3 grid(P, (lanes + 4 * kKv8Block - 1) / (4 * kKv8Block));   // up to four items per thread, as the f32 launch
    hipLaunchKernelGGL(kv8_rope_scatter, grid, dim3(kKv8Block), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_kv8_quantize_cache(const float *src, int8_t *dst, float *dst_s, int runs, int seq_len, int head_size, int n_pos,
                                     hipStream_t st)
{
    if (src == nullptr || dst == nullptr || dst_s == nullptr || runs < 1 || head_size < 4 || head_size > 256 || (head_size & 3) ||
        n_pos < 1 || n_pos > seq_len || (((uintptr_t)src) & 15) || (((uintptr_t)dst) & 3))
        return hipErrorInvalidValue;
    const size_t units = (size_t)runs * (size_t)n_pos, G = (size_t)(kKv8Block / kv8_lanes(head_size));
    const size_t blocks = (units + G - 1) / G;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kv8_quantize_cache, dim3((unsigned)blocks), dim3(kKv8Block), 0, st, src, dst, dst_s, units, seq_len, head_size, n_pos);
    return hipGetLastError();
}

}  // namespace l2z
