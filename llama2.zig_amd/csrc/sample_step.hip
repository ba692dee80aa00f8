// sample_step.hip -- l2z_sample_run's last node: the sampled sibling of argmax_kernel under `advance` (misc_kernels.hip).
// One block of 1024 threads draws the step's token from the runstate's logits with the shared row body (sample_device.h:
// the token l2z_sample_batch draws from the same logits, temperature, top_p and coin), then hands token, pos and the next
// embedding row over to the next replay of the step graph.
#include "q8_device.h"
#include "sample_device.h"

namespace l2z {
namespace {

__global__ __launch_bounds__(kSbThreads) void sample_step_kernel(const SampleStepArgs a)
{
    __shared__ SampleLds L;
    __shared__ int s_next;
    const int tid = threadIdx.x;
    const int pos = *a.pos_ptr;
    if (pos < 0 || pos >= a.seq_len) return;  // (the host never replays past seq_len; coins and out_tokens end there)
    const bool forced = pos < *a.n_prompt_ptr;  // :999-1000: the logits of a prompt position are never looked at
    int next = 0;
    if (!forced) next = sample_row(L, a.logits, a.vocab, a.params->temperature, a.params->top_p, a.coins[pos], a.scratch);
    __syncthreads();  // every thread has read pos before thread 0 moves it on
    if (tid == 0) {
        if (forced) next = a.prompt[pos];
        // Unreachable by construction: sample_row returns an index it scanned or a candidate's id, l2z_greedy_begin has
        // checked the prompt.  Kept, as argmax_kernel keeps its own, so that no id can ever address past the embedding table
        if ((unsigned)next >= (unsigned)a.vocab) next = 0;
        a.out_tokens[pos] = next;
        *a.token_ptr = next;   // :1036
        *a.pos_ptr = pos + 1;  // :995
        s_next = next;
    }
    __syncthreads();
    // next step's embedding row -> x (main.zig:295-296)
    if (a.emb_q8.q != nullptr) {
        q8_embed_row(a.emb_q8, s_next, a.dim, a.x, tid, kSbThreads);
        return;
    }
    const float *row = a.tok_emb + (size_t)s_next * (size_t)a.dim;
    for (int i = tid; i < a.dim; i += kSbThreads) a.x[i] = row[i];
}

}  // namespace

hipError_t launch_sample_step(const SampleStepArgs &a, hipStream_t st)
{
    if (a.vocab < 1 || a.dim < 1 || a.seq_len < 1 || a.params == nullptr || a.coins == nullptr || a.scratch == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_step_kernel, dim3(1), dim3(kSbThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace l2z
