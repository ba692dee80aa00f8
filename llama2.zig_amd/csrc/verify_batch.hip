// verify_batch.hip -- the kernels l2z_verify_batch adds to the batched step (host side: verify_host.cpp): the verify pass
// of verify.hip for the rows of SEVERAL sequences at once.  Group j of VerifyGroupTable is one sequence's consecutive
// positions on that sequence's own cache; attention, combine and verdict run per group in one launch each.
//
// The defining property (include/llama2_hip_test.h): a sequence's rows come out bit-identical to l2z_verify's on the same
// state.  The attention and combine bodies are verify.hip's own text (verify_device.h) applied to the group's rows, its
// pos0 and its cache; nothing a block computes looks at another group, at the number of groups or at the group's place.
#include "batch_decode.h"
#include "kernel_common.h"
#include "verify_device.h"

namespace l2z {
namespace {

// Block (h, seg, group).  The grid's y extent is the DEEPEST group's segment count: a block past its own group's last
// segment has no key to look at and returns (uniformly, before any barrier).
__global__ __launch_bounds__(kVaBlock) void verify_batch_attention_kernel(const VerifyBatchAttnArgs b)
{
    __shared__ __attribute__((aligned(16))) float sc[seg_lds_floats<kBatchMax>];
    const int grp = blockIdx.z, seg = blockIdx.y;
    const VerifyGroupTable *gt = b.groups;
    const int first = gt->first[grp], n = gt->count[grp], pos0 = gt->pos0[grp];
    if (seg > (pos0 + n - 1) / kVerifySeg) return;
    VerifyAttnArgs a;  // the group as a call of its own: its rows, its cache, its pos0
    static_cast<VerifyAttnGeom &>(a) = b;  // (out is the combine's: the body does not look at it)
    a.q += (size_t)first * b.ldq;
    a.part_o += (size_t)first * b.n_heads * b.seg_cap * b.head_size;
    a.part_ml += (size_t)first * b.n_heads * b.seg_cap * 2;
    a.kc = gt->kc[grp] + b.layer_off;
    a.vc = gt->vc[grp] + b.layer_off;
    a.pos0 = pos0;
    verify_attention_body(a, n, blockIdx.x, seg, sc);
}

// Block (h, row): the row's segments 0 .. pos / kVerifySeg, pos = the row's own position in the step's table
__global__ __launch_bounds__(64) void verify_batch_combine_kernel(const VerifyBatchAttnArgs b)
{
    const int i = blockIdx.y;
    verify_combine_store(b, blockIdx.x, i, b.tab->pos[i] / kVerifySeg + 1);
}

// Block (x, group): verify_accept_kernel per group.  Every block finds its group's accept length itself over the group's
// own rows (at most 15 compares), block x = 0 writes it to out[n_rows + group]; row first + a of the logits matrix -> the
// group's runstate.
__global__ __launch_bounds__(256) void verify_batch_accept_kernel(const BatchTable *tab, const VerifyGroupTable *gt,
                                                                  const float *logits, int vocab, int *out, int n_rows)
{
    __shared__ int s_a;
    const int grp = blockIdx.y;
    const int first = gt->first[grp], n = gt->count[grp];
    if (threadIdx.x == 0) {
        int acc = 0;
        while (acc + 1 < n && tab->tokens[first + acc + 1] == out[first + acc]) acc++;
        s_a = acc;
    }
    __syncthreads();
    const int acc = s_a;
    float *dst = gt->dst[grp];
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < vocab) dst[j] = logits[(size_t)(first + acc) * vocab + j];
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n_rows + grp] = acc;
}

bool verify_batch_args_ok(const VerifyBatchAttnArgs &a, int nseg)
{
    return verify_geom_ok(a, nseg) && a.n_heads >= 1 && a.tab != nullptr && a.groups != nullptr;
}

}  // namespace

hipError_t launch_verify_batch_attention(const VerifyBatchAttnArgs &a, int n_groups, int max_segments, hipStream_t st)
{
    if (!verify_batch_args_ok(a, max_segments) || n_groups < 1 || n_groups > kBatchMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(verify_batch_attention_kernel, dim3(a.n_heads, max_segments, n_groups), dim3(kVaBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_verify_batch_combine(const VerifyBatchAttnArgs &a, int n_rows, hipStream_t st)
{
    if (!verify_batch_args_ok(a, 1) || n_rows < 1 || n_rows > kBatchMax) return hipErrorInvalidValue;
    hipLaunchKernelGGL(verify_batch_combine_kernel, dim3(a.n_heads, n_rows), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_verify_batch_accept(const BatchTable *tab, const VerifyGroupTable *groups, const float *logits, int vocab,
                                      int *out, int n_rows, int n_groups, hipStream_t st)
{
    if (n_rows < 1 || n_rows > kBatchMax || n_groups < 1 || n_groups > n_rows || vocab < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(verify_batch_accept_kernel, dim3((vocab + 255) / 256, n_groups), dim3(256), 0, st, tab, groups, logits,
                       vocab, out, n_rows);
    return hipGetLastError();
}

}  // namespace l2z
