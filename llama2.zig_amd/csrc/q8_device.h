// q8_device.h -- device helpers of the int8 group-quantized decode (q8_matvec.hip): the group
// quantization of four values a lane with the group's maximum taken across lanes, and the embedding row of a quantized
// table.  Anonymous namespace, like kernel_common.h.
#pragma once
#include "kernel_common.h"

namespace l2z {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}

// One quotient of the rule: round(v / s) with the f32 division correctly rounded (never a multiplication by a
// reciprocal).  EVEN: the weight rule, round half to even (export.py's torch.round); else the activation rule, round half
// away from zero (runq.c's round) -- roundf of the f32 quotient itself.  s == 0 (an all-zero group): 0.
template <bool EVEN>
__device__ __forceinline__ int q8_quotient(float v, float s)
{
    if (!(s > 0.0f)) return 0;
    const float q = __fdiv_rn(v, s);
    return (int)(EVEN ? rintf(q) : roundf(q));
}

// Four consecutive values of a group of GS, held by one lane: the GS / 4 lanes of the group (8 or 16 consecutive lanes,
// aligned: inside one DPP row) take the maximum of |v| together, every one of them computes the same scale
// s = max / 127 and quantizes its own four values.  Returns them packed as one dword (value k in byte k); *scale: s.
// Every lane of the group must be active.
template <int GS, bool EVEN>
__device__ __forceinline__ int q8_quant4(v4f v, float *scale)
{
    static_assert(GS == 32 || GS == 64, "group sizes of the format");
    float m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
    m = fmaxf(m, dpp_mov<kDppXor1>(m));
    m = fmaxf(m, dpp_mov<kDppXor2>(m));
    m = fmaxf(m, dpp_mov<kDppHalfMirror>(m));
    if (GS == 64) m = fmaxf(m, dpp_mov<kDppMirror>(m));
    const float s = __fdiv_rn(m, 127.0f);
    *scale = s;
    const int q0 = q8_quotient<EVEN>(v.x, s), q1 = q8_quotient<EVEN>(v.y, s);
    const int q2 = q8_quotient<EVEN>(v.z, s), q3 = q8_quotient<EVEN>(v.w, s);
    return (q0 & 0xff) | ((q1 & 0xff) << 8) | ((q2 & 0xff) << 16) | (int)((unsigned)(q3 & 0xff) << 24);
}

// sum of an int over the aligned groups of N lanes (N = 2 or 4); every lane of the group gets it
template <int N>
__device__ __forceinline__ int q8_lanes_sum(int v)
{
    v += dpp_mov_i<kDppXor1>(v);
    if (N >= 4) v += dpp_mov_i<kDppXor2>(v);
    return v;
}

// row `token` of a quantized embedding table -> x, f32(q) * s: one rounding an element
__device__ __forceinline__ void q8_embed_row(const Q8Emb &e, int token, int dim, float *x, int tid, int n_threads)
{
    const size_t base = (size_t)token * (size_t)dim;
    for (int i = tid; i < dim; i += n_threads) {
        const size_t at = base + (size_t)i;
        x[i] = (float)e.q[at] * e.s[at / (size_t)e.gs];
    }
}

}  // namespace
}  // namespace l2z
