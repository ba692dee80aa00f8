// batch_decode.hip -- the kernels of the batched decode step that the prefill pass has no twin of: decode attention over
// n independent sequences (one block per (head, sequence), each reading its own cache up to its own position) and the
// per-row argmax.  The products run on the short-prompt GEMM forms (prefill_skinny.hip, G_*_ROWS epilogues).
#include "batch_decode.h"
#include "kernel_common.h"

namespace l2z {
namespace {

constexpr int kBaBlock = 256;
constexpr int kBaUB = 8;  // K / V rows a lane has in flight

// Block (h, b): head h of row b.  The row's K / V rows are head-major [kv head][seq_len][head_size] at
// tab->kc[b] + layer_off.  A row of K is read by TPR lanes (float4 each), R = 64 / TPR rows per wave side by side, so
// a wave-wide load is R whole rows -- contiguous.  Every order below (the lanes' partial dots, the groups' interleaved
// V sums, the block reductions) depends on the head size and the position alone: a row's output is the same bits
// whatever the other rows of the batch are.
__global__ __launch_bounds__(kBaBlock) void batch_attention_kernel(const BatchAttnArgs a)
{
    __shared__ __attribute__((aligned(16))) float qs[256];
    __shared__ __attribute__((aligned(16))) v4f part[kBaBlock];
    __shared__ float red[kBaBlock / 64];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int hs = a.head_size, E = hs >> 2;
    int TPR = 1;
    while (TPR < E) TPR <<= 1;
    const int G = kBaBlock / TPR, g = tid / TPR, c = tid % TPR;
    const int pos = a.tab->pos[b], T = pos + 1;
    const size_t head_off = a.layer_off + (size_t)(h / a.kv_mul) * a.kv_head_stride;
    const float *kbase = a.tab->kc[b] + head_off, *vbase = a.tab->vc[b] + head_off;
    float *att = a.scores + ((size_t)b * a.n_heads + h) * (size_t)a.seq_len;
    for (int i = tid; i < hs; i += kBaBlock) qs[i] = a.q[(size_t)b * a.ldq + (size_t)h * hs + i];
    __syncthreads();
    const v4f zero = {0.f, 0.f, 0.f, 0.f};
    const v4f qv = c < E ? ((const v4f *)qs)[c] : zero;
    const float div = sqrtf((float)hs);
    // scores att[t] = q . k_t / sqrt(head_size)   (:367-375; divide, not multiply by the reciprocal)
    float mx = -INFINITY;
    for (int t0 = g; t0 < T; t0 += G * kBaUB) {
        v4f kv[kBaUB];
#pragma unroll
        for (int i = 0; i < kBaUB; i++) {
            const int t = min(t0 + G * i, T - 1);  // clamped: result dropped below
            kv[i] = c < E ? ((const v4f *)(kbase + (size_t)t * hs))[c] : zero;
        }
#pragma unroll
        for (int i = 0; i < kBaUB; i++) {
            const float p = lanes_sum(hsum4(fma4(qv, kv[i], zero)), TPR);
            const int t = t0 + G * i;
            if (c == 0 && t < T) {
                const float s = p / div;
                att[t] = s;
                mx = fmaxf(mx, s);
            }
        }
    }
    mx = block_max(mx, red);  // (its barriers also publish att to the block)
    // softmax (:687-706): e^(s - max), the sum, then the divide
    float sum = 0.0f;
    for (int t = tid; t < T; t += kBaBlock) {
        const float e = expf(att[t] - mx);
        att[t] = e;
        sum += e;
    }
    sum = block_sum(sum, red);
    for (int t = tid; t < T; t += kBaBlock) att[t] = att[t] / sum;
    __syncthreads();
    // out = sum_t att[t] v_t   (:381-388): group g takes t = g, g + G, ... in increasing t; the groups combined in g order
    v4f acc = zero;
    for (int t0 = g; t0 < T; t0 += G * kBaUB) {
        v4f vv[kBaUB];
        float wt[kBaUB];
#pragma unroll
        for (int i = 0; i < kBaUB; i++) {
            const int t = min(t0 + G * i, T - 1);
            vv[i] = c < E ? ((const v4f *)(vbase + (size_t)t * hs))[c] : zero;
            wt[i] = att[t];
        }
#pragma unroll
        for (int i = 0; i < kBaUB; i++)
            if (t0 + G * i < T) {
                const v4f w4 = {wt[i], wt[i], wt[i], wt[i]};
                acc = fma4(w4, vv[i], acc);
            }
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < E) {
        v4f o = part[tid];
        for (int gg = 1; gg < G; gg++) o += part[gg * TPR + tid];
        *(v4f *)(a.out + (size_t)b * a.ldo + (size_t)h * hs + 4 * tid) = o;
    }
}

__global__ __launch_bounds__(1024) void batch_argmax_kernel(const BatchTable *tab, int vocab, int *out)
{
    __shared__ float s_val[16];
    __shared__ int s_idx[16];
    const int bi = block_argmax_1024(tab->logits[blockIdx.x], vocab, s_val, s_idx);
    if (threadIdx.x == 0) out[blockIdx.x] = bi;
}

}  // namespace

hipError_t launch_batch_attention(const BatchAttnArgs &a, int n, hipStream_t st)
{
    if (n < 1 || n > kBatchMax || a.head_size < 4 || a.head_size > 256 || (a.head_size & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(batch_attention_kernel, dim3(a.n_heads, n), dim3(kBaBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_batch_argmax(const BatchTable *tab, int vocab, int *out, int n, hipStream_t st)
{
    if (n < 1 || n > kBatchMax || vocab < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(batch_argmax_kernel, dim3(n), dim3(1024), 0, st, tab, vocab, out);
    return hipGetLastError();
}

}  // namespace l2z
