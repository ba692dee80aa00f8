// argmax_rule.h -- the one argmax rule of the decode path as every kernel applies it: the fused classifier epilogue
// (matvec.hip), argmax_kernel and its candidate exchange (misc_kernels.hip), the batched and verified rows
// (batch_decode.h) and the wide step's rows (wide_decode.hip); score.hip's top-1 states the same rule on its own
// partials.  They must all pick the same token, on every row of f32 values -- a NaN, an infinity, a signed zero and a
// denormal included.
//
// THE RULE is what the reference's scan returns (main.zig:715-726: max = x[0], then a strict '>' scan; a compare with a
// NaN on either side is false):
//   index 0                                          if x[0] is a NaN (nothing is ever greater than it);
//   the lowest index of the largest non-NaN value    otherwise (a NaN behind index 0 is never greater than the maximum);
//   index 0                                          if the row holds no non-NaN value.
// A candidate never holds a NaN.  It is EMPTY (-inf, kNoCandidate: no element yet, or only NaNs behind index 0), a
// non-NaN value with its index, or THE NaN AT INDEX 0, kept as (+inf, kNanFirst): no value is larger and no index lower,
// so it wins every merge, as an empty candidate -- no value smaller, no index higher -- loses every one.  The merge is
// then "larger value, else lower index" and nothing more; argmax_token turns the two special indices into token 0.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace l2z {

constexpr int kNoCandidate = 0x7fffffff;  // index of a candidate that has taken no element yet
constexpr int kNanFirst = -1;             // index of the candidate that stands for a NaN in element 0 of the row

struct ArgmaxCand {
    float v = -INFINITY;
    int i = kNoCandidate;
};

// Take element i of a row.  A row is always taken in INCREASING index order, so strict '>' keeps the lowest index of
// equal values (:720); the first non-NaN element is taken whatever its value (-inf included: it equals the empty
// candidate's value).  A NaN is passed over (both compares are false) -- except as element 0 of the row, which no later
// element displaces.
__device__ __forceinline__ void argmax_take(ArgmaxCand &c, float v, int i)
{
    if (v > c.v || (v == c.v && c.i == kNoCandidate)) {
        c.v = v;
        c.i = i;
    }
    if (i == 0 && v != v) {
        c.v = INFINITY;
        c.i = kNanFirst;
    }
}

// Merge another candidate (any order of indices): larger value wins, equal values -> lower index.  (The NaN at index 0
// and the empty candidate are the two ends of that order.)
__device__ __forceinline__ void argmax_merge(ArgmaxCand &c, float ov, int oi)
{
    if (ov > c.v || (ov == c.v && oi < c.i)) {
        c.v = ov;
        c.i = oi;
    }
}

// the token of a finished candidate: its index; 0 for the NaN at index 0 and for a row with no non-NaN value
__device__ __forceinline__ int argmax_token(const ArgmaxCand &c)
{
    return (unsigned)c.i >= (unsigned)kNoCandidate ? 0 : c.i;  // (kNanFirst is above it as an unsigned)
}

// xor-shuffle fold over the wave: every lane ends with the wave's candidate
__device__ __forceinline__ void argmax_wave_fold(ArgmaxCand &c)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(c.v, o, 64);
        const int oi = __shfl_xor(c.i, o, 64);
        argmax_merge(c, ov, oi);
    }
}

// c = wave 0's candidate; merges the candidates waves 1 .. nw - 1 left in LDS, in wave order
__device__ __forceinline__ void argmax_fold_waves(ArgmaxCand &c, const float *s_val, const int *s_idx, int nw)
{
    for (int w = 1; w < nw; w++) argmax_merge(c, s_val[w], s_idx[w]);
}

}  // namespace l2z
