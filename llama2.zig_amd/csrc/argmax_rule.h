// argmax_rule.h -- the one argmax rule of the decode path (main.zig:715-726: a strict '>' scan, so the FIRST maximum
// wins) as every kernel applies it: the fused classifier epilogue (matvec.hip), argmax_kernel and its candidate
// exchange (misc_kernels.hip) and the batched rows (batch_decode.h).  They must all pick the same token.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace l2z {

constexpr int kNoCandidate = 0x7fffffff;  // index of a candidate that has taken no element yet

struct ArgmaxCand {
    float v = -INFINITY;
    int i = kNoCandidate;
};

// Take element i of a row.  A row is always taken in INCREASING index order, so strict '>' keeps the lowest index of
// equal values (:720); the first element is taken whatever its value (-inf included).
__device__ __forceinline__ void argmax_take(ArgmaxCand &c, float v, int i)
{
    if (v > c.v || c.i == kNoCandidate) {
        c.v = v;
        c.i = i;
    }
}

// Merge another candidate (any order of indices): larger value wins, equal values -> lower index.
__device__ __forceinline__ void argmax_merge(ArgmaxCand &c, float ov, int oi)
{
    if (oi != kNoCandidate && (c.i == kNoCandidate || ov > c.v || (ov == c.v && oi < c.i))) {
        c.v = ov;
        c.i = oi;
    }
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
