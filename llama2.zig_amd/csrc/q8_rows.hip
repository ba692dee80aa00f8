// q8_rows.hip -- the row launches of the batched prompt pass on int8 group-quantized weights: the
// tokens' rows of the quantized embedding table into the residual matrix, and the group quantization of a chunk's rows
// -- after the rmsnorm where the product that follows has one -- into the int8 rows and scales the GEMM reads
// (q8_gemm.hip).  One block a row.  Compiled with -ffp-contract=off like every kernel file.
//
// The arithmetic of a row is the decode prologue's (q8_matvec.hip q8_stage_x), statement by statement and with the same
// block of 256 threads: the sum of squares by the same strided loop and block_sum, the same (v * s) * g, q8_device.h's
// rule on four values a lane.  A row quantized here has the bits the stepped pass gives the same row.
#include "q8_device.h"

namespace l2z {
namespace {

__global__ __launch_bounds__(kBlock) void q8_embed_rows_kernel(const Q8Emb e, const int *__restrict__ tokens, int dim,
                                                               float *__restrict__ x, int pos0, int *row_seq, int *row_pos)
{
    const int row = blockIdx.x;
    q8_embed_row(e, tokens[row], dim, x + (size_t)row * (size_t)dim, threadIdx.x, kBlock);
    if (threadIdx.x == 0 && row_seq != nullptr) {
        row_seq[row] = 0;
        row_pos[row] = pos0 + row;
    }
}

// row blockIdx.x of x -> n / 4 packed dwords and n / GS scales; rows m .. gridDim.x - 1 (the GEMM's pad): zeros
template <int GS>
__global__ __launch_bounds__(kBlock) void q8_quantize_rows_kernel(const float *__restrict__ x, int ldx, int m, int n,
                                                                  const float *__restrict__ rms_w, int *__restrict__ q,
                                                                  float *__restrict__ s)
{
    constexpr int L4 = GS / 4;  // lanes that hold a group
    __shared__ float scratch[kScratch];
    const int row = blockIdx.x, tid = threadIdx.x, n4 = n >> 2, ng = n / GS;
    int *xq = q + (size_t)row * (size_t)n4;
    float *xsc = s + (size_t)row * (size_t)ng;
    if (row >= m) {
        for (int j = tid; j < n4; j += kBlock) xq[j] = 0;
        for (int j = tid; j < ng; j += kBlock) xsc[j] = 0.0f;
        return;
    }
    const v4f *x4 = (const v4f *)(x + (size_t)row * (size_t)ldx), *g4 = (const v4f *)rms_w;
    const bool norm = rms_w != nullptr;
    float f = 1.0f;
    if (norm) {  // main.zig:432-468
        float ss = 0.0f;
        for (int j = tid; j < n4; j += kBlock) {
            const v4f v = x4[j];
            ss = fmaf(v.x, v.x, ss);
            ss = fmaf(v.y, v.y, ss);
            ss = fmaf(v.z, v.z, ss);
            ss = fmaf(v.w, v.w, ss);
        }
        const float tot = block_sum(ss, scratch);
        f = tot / (float)n;
        f += 1e-5f;
        f = 1.0f / sqrtf(f);
    }
    // n4 is a multiple of L4 and L4 divides 64: the lanes of a group are all in the loop together
    for (int j = tid; j < n4; j += kBlock) {
        v4f v = x4[j];
        if (norm) {
            const v4f g = g4[j];
            v.x = (v.x * f) * g.x;
            v.y = (v.y * f) * g.y;
            v.z = (v.z * f) * g.z;
            v.w = (v.w * f) * g.w;
        }
        float sc;
        xq[j] = q8_quant4<GS, false>(v, &sc);
        if ((tid % L4) == 0) xsc[j / L4] = sc;
    }
}

}  // namespace

hipError_t launch_q8_embed_rows(const Q8Emb &emb, const int *tokens, int dim, int P, float *x, int pos0, int *row_seq,
                                int *row_pos, hipStream_t st)
{
    if (emb.q == nullptr || emb.s == nullptr || (emb.gs != 32 && emb.gs != 64) || tokens == nullptr || x == nullptr || dim <= 0 ||
        P <= 0 || (row_seq == nullptr) != (row_pos == nullptr))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(q8_embed_rows_kernel, dim3(P), dim3(kBlock), 0, st, emb, tokens, dim, x, pos0, row_seq, row_pos);
    return hipGetLastError();
}

hipError_t launch_q8_quantize_rows(const float *x, int ldx, int m, int n, const float *rms_w, int gs, int8_t *q, float *s,
                                   hipStream_t st)
{
    if ((gs != 32 && gs != 64) || m <= 0 || n <= 0 || n % gs != 0 || ldx < n || (ldx & 3) != 0 || x == nullptr || q == nullptr ||
        s == nullptr)
        return hipErrorInvalidValue;
    // 16-byte loads of the rows and of the norm's weight, dword stores of the values
    if (!aligned16(x) || (rms_w != nullptr && !aligned16(rms_w)) || ((uintptr_t)q & 3u) != 0) return hipErrorInvalidValue;
    const dim3 grid(q8_gemm_rows_padded(m));
    if (gs == 32)
        hipLaunchKernelGGL(q8_quantize_rows_kernel<32>, grid, dim3(kBlock), 0, st, x, ldx, m, n, rms_w, (int *)q, s);
    else
        hipLaunchKernelGGL(q8_quantize_rows_kernel<64>, grid, dim3(kBlock), 0, st, x, ldx, m, n, rms_w, (int *)q, s);
    return hipGetLastError();
}

}  // namespace l2z
