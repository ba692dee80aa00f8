// kv8_layout.h -- the int8 KV cache of a runstate made by l2z_runstate_init_kv8.  Plain C++: no HIP,
// nothing of the library, like q8_layout.h.
//
// The unit is one kv head's slice of one position: head_size values and ONE f32 scale.  The rule is the ACTIVATION rule
// of q8_device.h over the slice -- s = max|v| / 127 (one correctly rounded f32 division), q = roundf(v / s) (one more);
// an all-zero slice has s = 0 and zeros -- applied to the f32 value the f32 cache would have held: K after RoPE, V as
// produced.  A reader sees f32(q) * s: one rounding.
// The arrays keep the f32 cache's head-major order:
//   K8, V8  int8  [layer][kv head][seq_len][head_size]
//   KS, VS  f32   [layer][kv head][seq_len]
// so the VALUE at (layer, kv head, t, i) stands at the element index the f32 cache gives the float, and its scale at
// that index without the innermost dimension.
#pragma once
#include <cstddef>
#include <cstdint>

namespace l2z {
namespace kv8 {

struct Dims {
    int n_layers, n_kv_heads, seq_len, head_size;
};

// head sizes the format's kernels take: a lane holds four values (one dword), at most 64 lanes a slice
inline bool head_size_ok(int hs) { return hs >= 4 && hs <= 256 && (hs & 3) == 0; }

inline size_t scales(const Dims &d) { return (size_t)d.n_layers * (size_t)d.n_kv_heads * (size_t)d.seq_len; }
inline size_t values(const Dims &d) { return scales(d) * (size_t)d.head_size; }
// bytes of the four arrays together, beside the 2 * values * 4 of the f32 caches
inline size_t bytes(const Dims &d) { return 2 * (values(d) + scales(d) * 4); }

inline size_t scale_at(const Dims &d, int layer, int kv_head, int t)
{
    return ((size_t)layer * (size_t)d.n_kv_heads + (size_t)kv_head) * (size_t)d.seq_len + (size_t)t;
}
inline size_t value_at(const Dims &d, int layer, int kv_head, int t, int i)
{
    return scale_at(d, layer, kv_head, t) * (size_t)d.head_size + (size_t)i;
}

}  // namespace kv8
}  // namespace l2z
