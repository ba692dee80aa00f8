// rope_device.h -- RoPE of four consecutive features of one head, as a lane of a row-per-lane epilogue holds them: the
// rotation of the prompt pass's scatter launch (prefill_ragged.hip) and of the q8 batched step's q | k | v epilogue
// (q8_batch.hip), one set of statements.  Compiled with -ffp-contract=off: no fused multiply-add.
#pragma once
#include <hip/hip_runtime.h>

namespace l2z {
namespace {

typedef float rope_v4f __attribute__((ext_vector_type(4)));   // (the kernel files' v4f)

// two pairs (main.zig:346-349): (v0, v1) -> (v0 c - v1 s, v0 s + v1 c) with cs = {c0, s0, c1, s1}
__device__ __forceinline__ rope_v4f rope_rotate4(rope_v4f x, rope_v4f cs)
{
    rope_v4f r;
    r.x = x.x * cs.x - x.y * cs.y; r.y = x.x * cs.y + x.y * cs.x;
    r.z = x.z * cs.z - x.w * cs.w; r.w = x.z * cs.w + x.w * cs.z;
    return r;
}

// cs of features f .. f + 3 of a row (f and head_size multiples of 4) at position pos; rope: (seq_len, head_size / 2)
// {cos, sin}, 16-byte aligned
__device__ __forceinline__ rope_v4f rope_cs4(const float2 *rope, int pos, int hs, int f)
{
    return *(const rope_v4f *)(rope + (size_t)pos * (size_t)(hs >> 1) + ((f % hs) >> 1));
}

}  // namespace
}  // namespace l2z
