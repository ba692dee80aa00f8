// batch_decode.h -- kernels of the batched decode step (batch_decode.hip; host side: batch_host.cpp).  One row per
// independent sequence: every row's position, KV caches and logits come from a small device table.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace l2z {

constexpr int kBatchMax = 16;  // L2Z_BATCH_MAX

// What the host uploads before a step, in one copy from a pinned buffer.  Cache bases are layer 0's; a launch adds
// its layer's offset.
struct BatchTable {
    int32_t tokens[kBatchMax];
    int32_t pos[kBatchMax];
    float *kc[kBatchMax];
    float *vc[kBatchMax];
    float *logits[kBatchMax];
};

// Decode attention (main.zig:361-389) for n rows, one block per (head, row): row b reads its own caches up to
// pos[b].  q: [n, ldq] (RoPE applied); out: [n, ldo]; scores: [n, n_heads, seq_len] scratch.
struct BatchAttnArgs {
    const float *q;
    float *out;
    float *scores;
    const BatchTable *tab;
    size_t layer_off;       // floats per layer of a cache
    size_t kv_head_stride;  // seq_len * head_size (head-major caches)
    int ldq, ldo, n_heads, kv_mul, head_size, seq_len;
};
hipError_t launch_batch_attention(const BatchAttnArgs &a, int n, hipStream_t st);

// out[b] = argmax of tab->logits[b][0 .. vocab) (main.zig:715-726: strict '>', lowest index wins), one block per row
hipError_t launch_batch_argmax(const BatchTable *tab, int vocab, int *out, int n, hipStream_t st);

}  // namespace l2z
