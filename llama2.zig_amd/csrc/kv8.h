// kv8.h -- the launches of the int8 KV cache (kv8_layout.h): the write side (kv8_scatter.hip: RoPE, the
// slice quantization and the scatter of a chunk's rows; the conversion of f32 cache rows behind l2z_runstate_fork) and the
// read side (kv8_attention.hip: decode attention of up to kWideMax one-row sequences over int8 rows;
// kv8_prefill_attention.hip: causal attention of a prompt chunk over one sequence's int8 rows; kv8_verify_attention.hip:
// that of up to kBatchMax guessed rows, a segment's bytes read once for all of them).  Host side: kv8_host.cpp,
// wide_host.cpp, q8_host.cpp (l2z_prefill_kv8, l2z_verify_kv8's pass), verify_host.cpp (l2z_verify_kv8).
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

// ---- the verify attention over int8 rows (kv8_verify_attention.hip) ----
// Causal attention of rows 0 .. n - 1 (n = L.P <= kBatchMax) of q [n, ldq] (RoPE applied; row i at position pos0 + i) of ONE
// sequence, seq8[seq] (device), over its rows 0 .. pos0 + n - 1 into out [n, ldo], two launches: kv8_verify_attention --
// block (kv head, segment) reads the segment's bytes and scales once and serves every row and every query head of the kv
// head from them, the flash partials per (row, head, segment) in wa.part, the wide step's layout -- and wide_combine as it
// stands (wa.tab->pos[i] = pos0 + i; wa.n_seg = the segments up to pos0 + n - 1).  Row i's bits are those launch_kv8_attention
// leaves for a one-row sequence at pos0 + i.  Keys beyond pos0 + n - 1 are never read, nor their scales; a key between a
// row's position and pos0 + n - 1 is read and does not reach that row.  hipErrorInvalidValue as launch_kv8_attention
hipError_t launch_kv8_verify_attention(const RaggedLayer &L, const WideAttn &wa, const Kv8Seq *seq8, int seq, int pos0,
                                       bool *planes_written = nullptr);

// ---- the prompt attention over int8 rows (kv8_prefill_attention.hip) ----
// The ONE sequence of a prompt chunk as the two forms find it: its arrays (the matrix-core form's kernel arguments) and, on
// the device, what the row form's launches read -- kWideMax slots that all name the sequence (slot 0 is also what
// launch_kv8_rope_scatter reads over a one-sequence table), then a WideTable per slice of kWideMax rows, of which pos[j] =
// pos0 + kWideMax * i + j alone is read -- and the wide step's partials.  kv8_prompt_tables fills the host image of slots
// and tables for a chunk, in that order, kv8_prompt_table_bytes of it (with_rows false: the slots alone).
struct Kv8Prompt {
    Kv8Seq seq;
    const Kv8Seq *slots;     // device: [kWideMax]
    const WideTable *tab;    // device: [ceil(P / kWideMax)]
    float *part;             // wide_part_floats
    int seg_cap;             // verify_segments(seq_len)
};
inline size_t kv8_prompt_table_bytes(int P, bool with_rows)
{
    return kWideMax * sizeof(Kv8Seq) + (with_rows ? (size_t)((P + kWideMax - 1) / kWideMax) * sizeof(WideTable) : 0);
}
void kv8_prompt_tables(void *host, const Kv8Seq &seq, int pos0, int P, bool with_rows);
// the matrix-core form's shape rule: head_size 64 or 128 and more than 32 rows; everything else takes the row form
bool kv8_prefill_flash_shape(int head_size, int P);
// Causal attention of rows 0 .. P - 1 of q [P, ldq] (RoPE applied; row i at position pos0 + i) over rows 0 .. pos0 + P - 1
// of seq8's arrays into out [P, ldo].  form 0: by kv8_prefill_flash_shape; 1: the row form -- launch_kv8_attention over
// slices of at most kWideMax rows, a row's arithmetic the wide step's own --; 3: the matrix-core form (hipErrorInvalidValue
// where its shape rule does not hold).  The matrix-core form loads whole tiles of 64 rows, clamped to row seq_len - 1: rows
// beyond a query's position are read and their bytes and scales may be anything; the result does not depend on them.
// layer_off / kv_head_stride: in VALUES
hipError_t launch_kv8_prefill_attention(const float *q, int ldq, const Kv8Prompt &seq8, float *out, int ldo, int pos0, int P,
                                        int n_heads, int head_size, int kv_mul, int seq_len, size_t layer_off, size_t kv_head_stride,
                                        hipStream_t st, int form = 0);

}  // namespace l2z
