// kv8.h -- the launches of the int8 KV cache (kv8_layout.h): the write side (kv8_scatter.hip: RoPE, the
// slice quantization and the scatter of a chunk's rows; the conversion of f32 cache rows behind l2z_runstate_fork) and the
// read side (kv8_attention.hip: decode attention of up to kWideMax one-row sequences over int8 rows).  Host side:
// kv8_host.cpp, wide_host.cpp.
#pragma once
#include "wide_decode.h"

namespace l2z {

// One sequence's four arrays (layer 0's bases), the twin of RaggedSeq's kc / vc in a wide table: slot j of the array that
// stands behind the WideTable is sequence j's
struct Kv8Seq {
    int8_t *k8, *v8;   // [layer][kv head][seq_len][head_size]
    float *ks, *vs;    // [layer][kv head][seq_len]
};

// launch_ragged_rope_scatter's contract over the same table, into int8 caches: q [P, dim] rotated in place (the f32
// scatter's bits), row r's K slices rotated, every K and V slice quantized by the activation rule over head_size and stored
// at row rg.row_pos[r] of sequence rg.row_seq[r]'s arrays seq8[..].  layer_off / kv_head_stride: in VALUES (the f32
// launch's numbers); seq_len: a kv head's scales
hipError_t launch_kv8_rope_scatter(float *q, int ldq, const RaggedChunk &rg, const Kv8Seq *seq8, int P, int dim, int kv_dim,
                                   int head_size, int seq_len, const float2 *rope, size_t layer_off, size_t kv_head_stride,
                                   hipStream_t st);

// rows 0 .. n_pos - 1 of every (layer, kv head) run of an f32 cache [runs][seq_len][head_size] -> the int8 array and its
// scales, by the scatter's slice function (the rows hold what the rule takes: K after RoPE, V as produced)
hipError_t launch_kv8_quantize_cache(const float *src, int8_t *dst, float *dst_s, int runs, int seq_len, int head_size, int n_pos,
                                     hipStream_t st);

// launch_wide_attention's contract over int8 rows, two launches: kv8_attention -- block (kv head x part of up to 4 query
// heads, segment, row), the flash partials per (row, head, segment) in wa.part -- and wide_combine as it stands.  seq8:
// device, slot i = row i.  Keys beyond wa.tab->pos[i] are never read, nor their scales.
hipError_t launch_kv8_attention(const RaggedLayer &L, const WideAttn &wa, const Kv8Seq *seq8, bool *planes_written = nullptr);

}  // namespace l2z
