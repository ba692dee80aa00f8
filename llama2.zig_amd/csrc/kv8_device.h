// kv8_device.h -- the two device functions of the int8 KV cache's format (kv8_layout.h), each ONCE: the
// slice quantization of the write side (kv8_scatter.hip: the scatter and the fork's conversion both call it) and the exact
// conversion of a dword of four values back to f32 on the read side (kv8_attention.hip).  Anonymous namespace, like
// q8_device.h, whose quotient rule this is.
#pragma once
#include "q8_device.h"

namespace l2z {
namespace {

// lanes a slice of head_size values stands in, a dword (four values) a lane: the next power of two from head_size / 4 up,
// so an aligned group of them never leaves a wave (12 lanes at head_size 48 stand in 16, the last four idle)
__host__ __device__ inline int kv8_lanes(int head_size)
{
    int tpr = 1;
    while (tpr < (head_size >> 2)) tpr <<= 1;
    return tpr;
}

// max over aligned groups of n lanes (a power of two up to 64), every lane gets it: lanes_sum's exchanges
__device__ __forceinline__ float kv8_lanes_max(float v, int n)
{
    if (n >= 2) v = fmaxf(v, dpp_mov<kDppXor1>(v));
    if (n >= 4) v = fmaxf(v, dpp_mov<kDppXor2>(v));
    if (n >= 8) v = fmaxf(v, dpp_mov<kDppHalfMirror>(v));
    if (n >= 16) v = fmaxf(v, dpp_mov<kDppMirror>(v));
    if (n >= 32) v = fmaxf(v, __shfl_xor(v, 16, 64));
    if (n >= 64) v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}

// THE slice function: four consecutive values of a slice a lane, the slice in an aligned group of tpr lanes (an idle lane
// of the group brings zeros, which leave the maximum alone).  The group takes max|v| together, every lane forms the same
// s = max / 127 and quantizes its own four values by the activation rule (q8_quotient<false>: roundf of the correctly
// rounded f32 quotient; s == 0: zeros).  Returns the values packed, value k in byte k; *scale: s.  Every lane of the
// group must be active.
__device__ __forceinline__ int kv8_quant_slice(v4f v, int tpr, float *scale)
{
    float m = fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
    m = kv8_lanes_max(m, tpr);
    const float s = __fdiv_rn(m, 127.0f);
    *scale = s;
    const int q0 = q8_quotient<false>(v.x, s), q1 = q8_quotient<false>(v.y, s);
    const int q2 = q8_quotient<false>(v.z, s), q3 = q8_quotient<false>(v.w, s);
    return (q0 & 0xff) | ((q1 & 0xff) << 8) | ((q2 & 0xff) << 16) | (int)((unsigned)(q3 & 0xff) << 24);
}

// the four values of a dword as f32, exactly (an int8 is a f32)
__device__ __forceinline__ v4f kv8_unpack(int w)
{
    const unsigned u = (unsigned)w;
    v4f r;
    r.x = (float)((int)(u << 24) >> 24);
    r.y = (float)((int)(u << 16) >> 24);
    r.z = (float)((int)(u << 8) >> 24);
    r.w = (float)(w >> 24);
    return r;
}

}  // namespace
}  // namespace l2z
