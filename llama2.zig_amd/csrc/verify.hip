// verify.hip -- the kernels l2z_verify adds to the batched step (host side: verify_host.cpp): attention for n rows of ONE
// sequence at consecutive positions, and the verdict (per-row argmax, accept length, hand-over of the accepted logits).
// l2z_verify_sample runs the same pass; its rows' ids come from sample_batch_kernel (sample_batch.hip) instead of the
// argmax.  The argmax also serves the greedy passes of l2z_verify_batch and l2z_verify_tree.
//
// DRAFT INVARIANCE (include/llama2_hip.h): what a row at position p computes is a function of p and the tokens 0 .. p.
// Here that means: the segment grid is fixed in ABSOLUTE positions (kVerifySeg keys per segment), a key the row may not
// see contributes nothing -- its score is -inf, its weight exactly 0, its V row is skipped -- and every order (the lanes'
// partial dots, a wave's max and sum over the segment, a group's V rows in increasing t, the groups in g order, the
// segments in segment order) depends on head_size and the segment alone, never on pos0, n or the row's index.
#include "batch_decode.h"
#include "kernel_common.h"
#include "verify_device.h"

namespace l2z {
namespace {

// Block (h, seg): head h over the keys t of segment seg that the call's rows see (verify_device.h)
__global__ __launch_bounds__(kVaBlock) void verify_attention_kernel(const VerifyAttnArgs a, const int n)
{
    __shared__ __attribute__((aligned(16))) float sc[seg_lds_floats<kBatchMax>];  // scores [row][key], then the groups' V sums
    verify_attention_body(a, n, blockIdx.x, blockIdx.y, sc);
}

// Block (h, i): row i's segments 0 .. (pos0 + i) / kVerifySeg folded in segment order, then the divide (verify_device.h)
__global__ __launch_bounds__(64) void verify_combine_kernel(const VerifyAttnArgs a)
{
    const int i = blockIdx.y;
    verify_combine_store(a, blockIdx.x, i, (a.pos0 + i) / kVerifySeg + 1);
}

__global__ __launch_bounds__(1024) void verify_argmax_kernel(const float *logits, int vocab, int *out)
{
    __shared__ float s_val[16];
    __shared__ int s_idx[16];
    const int bi = block_argmax_1024(logits + (size_t)blockIdx.x * vocab, vocab, s_val, s_idx);
    if (threadIdx.x == 0) out[blockIdx.x] = bi;
}

// out[0 .. n) = the rows' next ids (verify_argmax_kernel, or sample_batch_kernel for a sampled pass).  Every block finds
// the accept length a itself (at most 15 compares), block 0 writes it to out[n]; row a of the logits matrix -> dst.
__global__ __launch_bounds__(256) void verify_accept_kernel(const BatchTable *tab, const float *logits, int vocab, int *out,
                                                            float *dst, int n)
{
    __shared__ int s_a;
    if (threadIdx.x == 0) {
        int acc = 0;
        while (acc + 1 < n && tab->tokens[acc + 1] == out[acc]) acc++;
        s_a = acc;
    }
    __syncthreads();
    const int acc = s_a;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < vocab) dst[j] = logits[(size_t)acc * vocab + j];
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = acc;
}

bool verify_args_ok(const VerifyAttnArgs &a, int n)
{
    return n >= 1 && n <= kBatchMax && a.pos0 >= 0 && verify_geom_ok(a, (a.pos0 + n - 1) / kVerifySeg + 1);
}

}  // namespace

hipError_t launch_verify_attention(const VerifyAttnArgs &a, int n, hipStream_t st)
{
    if (!verify_args_ok(a, n)) return hipErrorInvalidValue;
    const int nseg = (a.pos0 + n - 1) / kVerifySeg + 1;
    hipLaunchKernelGGL(verify_attention_kernel, dim3(a.n_heads, nseg), dim3(kVaBlock), 0, st, a, n);
    return hipGetLastError();
}

hipError_t launch_verify_combine(const VerifyAttnArgs &a, int n, hipStream_t st)
{
    if (!verify_args_ok(a, n)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(verify_combine_kernel, dim3(a.n_heads, n), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_verify_argmax(const float *logits, int vocab, int *out, int rows, hipStream_t st)
{
    if (rows < 1 || rows > kBatchMax || vocab < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(verify_argmax_kernel, dim3(rows), dim3(1024), 0, st, logits, vocab, out);
    return hipGetLastError();
}

hipError_t launch_verify_accept(const BatchTable *tab, const float *logits, int vocab, int *out, float *dst, int n,
                                hipStream_t st)
{
    if (n < 1 || n > kBatchMax || vocab < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(verify_accept_kernel, dim3((vocab + 255) / 256), dim3(256), 0, st, tab, logits, vocab, out, dst, n);
    return hipGetLastError();
}

}  // namespace l2z
