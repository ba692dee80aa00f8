// sample_batch.hip -- l2z_sample_batch's kernel: one token drawn per row from a runstate's logits, on the device, with
// the bits the host samplers give.  One block of 1024 threads per row runs the shared row body (sample_device.h); rows are
// independent, so a row's token depends on its own logits, temperature, top_p and coin alone.
#include "sample_device.h"

namespace l2z {
namespace {

__global__ __launch_bounds__(kSbThreads) void sample_batch_kernel(const SampleArgs a)
{
    __shared__ SampleLds L;
    const int b = blockIdx.x;
    const BatchTable *tab = a.tab;
    const int t = sample_row(L, tab->logits[b], a.vocab, tab->temperature[b], tab->top_p[b], tab->coin[b],
                             a.scratch + (size_t)b * a.row_stride);
    if (threadIdx.x == 0) a.out[b] = t;
}

}  // namespace

hipError_t launch_sample_batch(const SampleArgs &a, int n, hipStream_t st)
{
    if (n < 1 || n > kBatchMax || a.vocab < 1 || a.row_stride < sample_scratch_floats(a.vocab)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_batch_kernel, dim3(n), dim3(kSbThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace l2z
