// wide_sample.hip -- the last launch of one step of l2z_wide_run (wide_decode.h; host side: wide_host.cpp): every row's
// token drawn on the device by the sampler's shared row body (sample_device.h -- the token l2z_sample_batch draws from the
// same logits, temperature, top_p and coin; the argmax at temperature 0), and the row handed over to the next step's
// launches: its token to the embed launch, its position to the table the RoPE / scatter and attention launches read.
// One block of 1024 threads per row; no block touches two rows.  Vector loads and stores only.
#include "wide_decode.h"

#include "sample_device.h"

namespace l2z {
namespace {

__global__ __launch_bounds__(kSbThreads) void wide_draw_advance(const WideDraw a)
{
    __shared__ SampleLds L;
    const int row = blockIdx.x, tid = threadIdx.x;
    const float *lg = a.logits + (size_t)row * a.ld;
    const float temperature = a.temperature ? a.temperature[row] : 0.0f;
    const bool greedy = temperature == 0.0f;
    int next = sample_row(L, lg, a.vocab, temperature, greedy ? 0.0f : a.top_p[row], greedy ? 0.0f : a.coins[row],
                          greedy ? nullptr : a.scratch + (size_t)row * a.row_stride);
    if (a.logits_out) block_copy_row(a.tab->logits[row], lg, a.vocab, tid, kSbThreads);  // wide_logits_out's copy
    if (tid == 0) {
        // Unreachable by construction (sample_row returns an index it scanned or a candidate's id); kept, as
        // sample_step_kernel keeps its own, so that no id can ever address past the embedding table
        if ((unsigned)next >= (unsigned)a.vocab) next = 0;
        a.ids[row] = next;
        a.tokens[row] = next;
        // this block alone reads or writes row's entries, and the step's other launches are done with them
        a.tab->pos[row] += 1;
        a.tab->seq[row].pos0 += 1;
    }
}

}  // namespace

hipError_t launch_wide_draw_advance(const WideDraw &d, int n, hipStream_t st)
{
    const bool sampled = d.temperature != nullptr;
    if (n < 1 || n > kWideMax || d.vocab < 1 || d.ld < d.vocab || d.logits == nullptr || d.tab == nullptr || d.ids == nullptr ||
        d.tokens == nullptr)
        return hipErrorInvalidValue;
    if (sampled && (d.top_p == nullptr || d.coins == nullptr || d.scratch == nullptr || d.row_stride < sample_scratch_floats(d.vocab)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(wide_draw_advance, dim3(n), dim3(kSbThreads), 0, st, d);
    return hipGetLastError();
}

}  // namespace l2z
