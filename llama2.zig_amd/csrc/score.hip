// score.hip -- the reductions behind l2z_score: per token row, log-softmax at a target and the argmax over the vocabulary,
// from classifier logits that exist only one vocabulary SLAB at a time (prefill_host.cpp score_chunk: final rmsnorm of the
// chunk's residual rows, then [P, dim] x [slab rows of wcls, dim]^T by the prefill GEMM launchers into a workspace).
//
// The vocabulary is cut into SEGMENTS of kScoreSeg = 4096 columns, a property of the reduction alone: a slab is a whole
// number of segments (the last one of the vocabulary may be short), so the sums below and their order are functions of
// vocab_size only -- never of the slab width, the chunk length or the runstate's history.
//   score_reduce_kernel   one block of four waves per (token row, segment): a wave takes 1024 columns as four 16-byte
//                         loads per lane, keeps (max, first index of the max), combines across lanes (DPP / shuffles),
//                         sums exp(z - wave max) over its columns, and thread 0 folds the four waves' triples in wave order
//                         through LDS into the segment's (max, sum of exp relative to that max, first index of the max).
//                         The block whose segment holds the row's target column keeps that logit.
//   score_finish_kernel   one thread per token row folds the segments' triples in segment order (online log-sum-exp:
//                         a larger max rescales the running sum) and writes logprob = z[target] - (max + log(sum)), top1.
// Top-1 is l2z_argmax's rule (argmax_rule.h: what the scan of main.zig:715-726 returns).  A later column / lane / wave /
// segment replaces the running best only when strictly greater, equal maxima across lanes resolve to the lowest index,
// and a NaN is never greater than anything: the lowest index of the largest non-NaN value, index 0 if there is none.
// Column 0 of the vocabulary is the scan's first element and wins outright when it is a NaN: the block that owns it
// leaves kScoreNanFirst as its segment's index, which outlives every fold.  (The max and the sum behind the log-prob skip
// nothing: a row with a NaN has a NaN log-prob.)  exp is expf, as in block_softmax behind l2z_probs_read.  Compiled with -ffp-contract=off: every sum is a plain f32 add in the order written.
#include <climits>

#include "kernel_common.h"

namespace l2z {
namespace {

constexpr int kSegWaveCols = kScoreSeg / kWaves;       // 1024 columns per wave
constexpr int kSegLoads = kSegWaveCols / (4 * kWave);  // four 16-byte loads per lane
static_assert(kSegLoads * 4 * kWave * kWaves == kScoreSeg, "a segment is whole 16-byte loads of four waves");
constexpr int kScoreNanFirst = -1;  // part_i of the vocabulary's first segment: column 0 is a NaN, top-1 is 0

__device__ __forceinline__ int wave_min_int(int v)
{
    for (int d = 1; d < kWave; d <<= 1) v = min(v, __shfl_xor(v, d, kWave));
    return v;
}

// running (max m, sum s of exp relative to m, first index i of m) <- itself folded with a later part (pm, ps, pi)
__device__ __forceinline__ void fold(float &m, float &s, int &i, float pm, float ps, int pi)
{
    if (pm > m) {
        s = s * expf(m - pm) + ps;   // (m == -inf: s is 0 and stays 0 * 0)
        m = pm;
        i = pi;
    } else if (pm != -INFINITY) {
        s = s + ps * expf(pm - m);
    }
}

__global__ __launch_bounds__(kBlock) void score_reduce_kernel(const ScoreArgs a)
{
    __shared__ float sh_m[kWaves], sh_s[kWaves];
    __shared__ int sh_i[kWaves];
    const int seg = blockIdx.x, row = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float *z = a.slab + (size_t)row * a.ld;
    const int c0 = seg * kScoreSeg + wave * kSegWaveCols;   // first column of the wave, in the slab

    // the row pitch is a whole number of segments: every 16-byte load lies inside the row; columns >= a.n are not logits
    v4f v[kSegLoads];
#pragma unroll
    for (int j = 0; j < kSegLoads; j++) v[j] = *(const v4f *)(z + c0 + 4 * (lane + kWave * j));
    // thread 0 holds the segment's first column in v[0][0]: column 0 of the vocabulary in the first segment of the first slab
    const bool nan_first = a.col0 + seg * kScoreSeg == 0 && v[0][0] != v[0][0];
    float m = -INFINITY;
    int mi = INT_MAX;
#pragma unroll
    for (int j = 0; j < kSegLoads; j++) {
        const int c = c0 + 4 * (lane + kWave * j);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (c + e >= a.n) v[j][e] = -INFINITY;
            if (v[j][e] > m) { m = v[j][e]; mi = c + e; }
        }
    }
    const float wm = wave_max(m);
    const int wi = wave_min_int(m == wm ? mi : INT_MAX);
    float s = 0.0f;
    if (wm != -INFINITY) {
#pragma unroll
        for (int j = 0; j < kSegLoads; j++)
#pragma unroll
            for (int e = 0; e < 4; e++) s += expf(v[j][e] - wm);   // (columns past a.n: exp(-inf) = 0)
    }
    s = wave_sum(s);
    if (lane == 0) { sh_m[wave] = wm; sh_s[wave] = s; sh_i[wave] = wi; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float bm = -INFINITY, bs = 0.0f;
    int bi = INT_MAX;
    for (int w = 0; w < kWaves; w++) fold(bm, bs, bi, sh_m[w], sh_s[w], sh_i[w]);
    const size_t at = (size_t)row * a.nseg + a.seg0 + seg;
    a.part_m[at] = bm;
    a.part_s[at] = bs;
    a.part_i[at] = nan_first ? kScoreNanFirst : bi == INT_MAX ? 0 : a.col0 + bi;
    if (a.targets != nullptr) {
        const int t = a.targets[row] - a.col0;   // (no target: -1 - col0 < 0)
        const int end = min((seg + 1) * kScoreSeg, a.n);
        if (a.targets[row] >= 0 && t >= seg * kScoreSeg && t < end) a.tgt[row] = z[t];
    }
}

__global__ __launch_bounds__(kBlock) void score_finish_kernel(const ScoreArgs a)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= a.P) return;
    float m = -INFINITY, s = 0.0f;
    int i = 0;
    for (int g = 0; g < a.nseg; g++) {
        const size_t at = (size_t)row * a.nseg + g;
        fold(m, s, i, a.part_m[at], a.part_s[at], a.part_i[at]);
    }
    if (a.part_i[(size_t)row * a.nseg] == kScoreNanFirst) i = 0;
    if (a.out_top1 != nullptr) a.out_top1[row] = i;
    if (a.out_logprob != nullptr) {
        const bool has = a.targets != nullptr && a.targets[row] >= 0;
        a.out_logprob[row] = has ? a.tgt[row] - (m + logf(s)) : 0.0f;
    }
}

}  // namespace

hipError_t launch_score_reduce(const ScoreArgs &a, hipStream_t st)
{
    if (a.P < 1 || a.n < 1 || a.ld % kScoreSeg != 0 || a.n > a.ld || a.col0 % kScoreSeg != 0 || ((uintptr_t)a.slab & 15))
        return hipErrorInvalidValue;
    const int segs = (a.n + kScoreSeg - 1) / kScoreSeg;
    if (a.seg0 != a.col0 / kScoreSeg || a.seg0 + segs > a.nseg) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)segs, (unsigned)a.P), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_score_finish(const ScoreArgs &a, hipStream_t st)
{
    if (a.P < 1 || a.nseg < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_finish_kernel, dim3((unsigned)((a.P + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace l2z
