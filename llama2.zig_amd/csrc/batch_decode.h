// batch_decode.h -- the kernels that run on the batched step's rows, as the host sees them: the step's own attention and
// argmax (batch_decode.hip; host side batch_host.cpp), the row sampler (sample_batch.hip) and the verify family's
// attention forms and verdicts (verify.hip, verify_batch.hip, verify_tree.hip; host side verify_host.cpp).  Every row's
// token, position, KV caches and logits come from a small device table.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "argmax_rule.h"
#include "l2z_internal.h"

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
    float temperature[kBatchMax];  // l2z_sample_batch only
    float top_p[kBatchMax];
    float coin[kBatchMax];
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

// out[b] = argmax of tab->logits[b][0 .. vocab) by argmax_rule.h (main.zig:715-726: what the strict-'>' scan returns,
// NaN rows included), one block per row
hipError_t launch_batch_argmax(const BatchTable *tab, int vocab, int *out, int n, hipStream_t st);

// The argmax of lg[0 .. vocab) for a block of 1024 threads, valid in thread 0: each thread scans its indices in
// increasing order (strict '>' keeps the lowest, :720; a NaN counts only as element 0), the candidates combine by
// argmax_merge (value, then lower index; the NaN at index 0 above all); no non-NaN value: index 0.
// s_val / s_idx: 16 entries of LDS each.  Shared by the argmax of the batched step and l2z_sample_batch's rows at
// temperature 0, which must pick the same token.
__device__ inline int block_argmax_1024(const float *lg, int vocab, float *s_val, int *s_idx)
{
    const int tid = threadIdx.x;
    ArgmaxCand c;
    for (int i = tid; i < vocab; i += 1024) argmax_take(c, lg[i], i);
    argmax_wave_fold(c);
    if ((tid & 63) == 0) { s_val[tid >> 6] = c.v; s_idx[tid >> 6] = c.i; }
    __syncthreads();
    if (tid == 0) argmax_fold_waves(c, s_val, s_idx, 16);
    return argmax_token(c);
}

// The batched step on int8 group-quantized weights (q8_batch.hip): its two launches that read the table.
// Both multiply the step's m <= kBatchMax quantized rows (xq [16, n], xs [16, n / gs]: padded to the GEMM's tile, the pad
// rows zero, as launch_q8_quantize_rows leaves them) on the int8 matrix cores with launch_q8_gemm's arithmetic, bit for bit.
// q | k | v of a layer in one launch: q rows -> q [m, ldq] with RoPE at tab->pos[row]; the k row (RoPE) and the v row into
// tab->kc[row] / tab->vc[row] + layer_off, head-major, at the row's position.  dim, kvd, hs: the model's dim, kv_dim and
// head_size (hs a multiple of 4); w*_q / _k / _v: the layer's Wq [dim, n], Wk and Wv [kvd, n] and their scales
struct Q8BatchQkvArgs {
    const int8_t *xq;
    const float *xs;
    const int8_t *wq_q, *wq_k, *wq_v;
    const float *ws_q, *ws_k, *ws_v;
    float *q;
    const BatchTable *tab;
    const float2 *rope;
    size_t layer_off, kv_head_stride;
    int ldq, m, n, dim, kvd, hs, gs;
};
hipError_t launch_q8_batch_qkv(const Q8BatchQkvArgs &a, hipStream_t st);
// the classifier [vocab, n] (vocab a multiple of 4): row r's logits -> tab->logits[r][0 .. vocab), whole
struct Q8BatchClsArgs {
    const int8_t *xq;
    const float *xs;
    const int8_t *wq;
    const float *ws;
    const BatchTable *tab;
    int m, n, vocab, gs;
};
hipError_t launch_q8_batch_cls(const Q8BatchClsArgs &a, hipStream_t st);

// l2z_sample_batch (sample_batch.hip): row b draws one token from tab->logits[b] with tab->temperature[b],
// tab->top_p[b] and tab->coin[b] exactly as the host samplers do (llama2.zig_amd/host, main.zig:728-798), one block of
// 1024 threads per row.  scratch: sample_scratch_floats(vocab) floats per row, row_stride apart.
struct SampleArgs {
    const BatchTable *tab;
    float *scratch;
    size_t row_stride;
    int vocab;
    int *out;
};
inline size_t sample_scratch_floats(int vocab) { return 5 * (((size_t)vocab + 63) / 64 * 64); }
hipError_t launch_sample_batch(const SampleArgs &a, int n, hipStream_t st);

// l2z_sample_run (sample_step.hip): the last node of a sampled step graph, one block of 1024 threads -- argmax_kernel's
// hand-over (main.zig:999-1003, :1036) with the argmax replaced by the row body's draw from the runstate's logits.  What
// changes from step to step or from call to call is read from device memory, never from the arguments, which a captured
// graph freezes: pos from *pos_ptr, temperature and top_p from *params, the coin from coins[pos].
struct SampleStepParams {
    float temperature, top_p;
};
struct SampleStepArgs {
    const float *logits;             // read only: the step's logits stay as the classifier left them
    int vocab;
    const SampleStepParams *params;
    const float *coins;              // [seq_len], indexed by position; not read at a prompt position
    int seq_len;                     // a position outside [0, seq_len) is left alone: nothing is read or written
    float *scratch;                  // sample_scratch_floats(vocab) floats
    int *token_ptr;                  // out: the next step's token
    int *pos_ptr;                    // in/out
    const int *prompt;               // forced tokens (n_prompt)
    const int *n_prompt_ptr;
    int *out_tokens;                 // out_tokens[pos] = next
    const float *tok_emb;            // (vocab, dim): next step's embedding row -> x
    float *x;
    int dim;
    Q8Emb emb_q8;                    // q != null: the embedding table is the quantized one, tok_emb is not read
};
hipError_t launch_sample_step(const SampleStepArgs &a, hipStream_t st);

// The verify family (verify.hip, verify_batch.hip, verify_tree.hip; host side: verify_host.cpp): the rows of a step are
// guessed positions, attention is multi-query, causal and split over positions.  A block owns (head, segment), the
// segments are kVerifySeg ABSOLUTE positions each -- segment s = positions [s * kVerifySeg, (s + 1) * kVerifySeg) whatever
// the call's first position and row count are -- loads each K and V row of its segment once and uses it for every row; it
// leaves per (row, head, segment) the flash partials (max, sum e^(s - max), sum e^(s - max) v).  The combine folds a row's
// segments in segment order and divides.  Every order is a function of head_size, the segment and the row's position alone:
// the kernels are wrappers around the segment bodies of verify_device.h, which the wide step (wide_decode.h) runs too,
// there with the query heads of one row where these have the rows of one head.
constexpr int kVerifySeg = 64;
inline int verify_segments(int seq_len) { return (seq_len + kVerifySeg - 1) / kVerifySeg; }
// What the three attention forms share: the rows' queries, outputs and partials
struct VerifyAttnGeom {
    const float *q;    // [rows, ldq], RoPE applied
    float *out;        // [rows, ldo]
    float *part_o;     // [kBatchMax, n_heads, seg_cap, head_size]
    float *part_ml;    // [kBatchMax, n_heads, seg_cap, 2]: max, sum
    size_t kv_head_stride;
    int ldq, ldo, n_heads, kv_mul, head_size, seg_cap;
};

// l2z_verify, l2z_verify_sample (verify.hip): n rows of ONE sequence at consecutive positions tab->pos[i] = pos0 + i, all
// on one cache.
struct VerifyAttnArgs : VerifyAttnGeom {
    const float *kc, *vc;  // the layer's caches, head-major [kv head][seq_len][head_size]
    int pos0;
};
hipError_t launch_verify_attention(const VerifyAttnArgs &a, int n, hipStream_t st);
hipError_t launch_verify_combine(const VerifyAttnArgs &a, int n, hipStream_t st);

// The verdict of a verify pass, on the device, in two launches.  First the rows' next ids into out[0 .. rows): the argmax
// of logits + i * vocab (block_argmax_1024: the tie rule of l2z_argmax_batch) by launch_verify_argmax, or the draws of
// launch_sample_batch (tab->logits[i] = logits + i * vocab, out = the same out) for a sampled pass.  Then the form's own
// accept kernel.  The chain's: a = the number of leading guesses tab->tokens[j] == next[j - 1], j = 1 ..; out[n] = a; row
// a of the logits matrix is copied to dst (the runstate's logits).
hipError_t launch_verify_argmax(const float *logits, int vocab, int *out, int rows, hipStream_t st);
hipError_t launch_verify_accept(const BatchTable *tab, const float *logits, int vocab, int *out, float *dst, int n,
                                hipStream_t st);

// l2z_verify_batch (verify_batch.hip): the rows of a step are GROUPS of consecutive positions, one group per sequence --
// group j is rows first[j] .. first[j] + count[j] - 1 at positions pos0[j] .. of the sequence whose caches are kc[j] /
// vc[j] (layer 0's bases) and whose runstate logits are dst[j].  Uploaded behind the step's BatchTable in the same copy.
struct VerifyGroupTable {
    int32_t first[kBatchMax], count[kBatchMax], pos0[kBatchMax];
    float *kc[kBatchMax];
    float *vc[kBatchMax];
    float *dst[kBatchMax];
};
static_assert(sizeof(BatchTable) % alignof(VerifyGroupTable) == 0, "the group table sits right behind the step's table");
// Attention of every group in one launch per layer: block (head, segment, group) runs verify_attention_kernel's body
// (verify_device.h) on the group's rows and the group's cache, so a row's partials are the bits l2z_verify leaves for
// it.  The grid is (n_heads, max_segments, n_groups), max_segments = the deepest group's segment count; a block past
// its own group's last segment returns at once.  Partials are indexed by the row's place in the step; the combine takes
// a row's segment count from tab->pos[row].
struct VerifyBatchAttnArgs : VerifyAttnGeom {
    const BatchTable *tab;
    const VerifyGroupTable *groups;
    size_t layer_off;  // floats per layer of a cache
};
hipError_t launch_verify_batch_attention(const VerifyBatchAttnArgs &a, int n_groups, int max_segments, hipStream_t st);
hipError_t launch_verify_batch_combine(const VerifyBatchAttnArgs &a, int n_rows, hipStream_t st);
// The verdict per group: group j's accept length a_j over its own rows (tab->tokens against out[0 .. n_rows), the rows'
// next ids) -> out[n_rows + j]; row first[j] + a_j of the logits matrix -> groups->dst[j].  One launch.
hipError_t launch_verify_batch_accept(const BatchTable *tab, const VerifyGroupTable *groups, const float *logits, int vocab,
                                      int *out, int n_rows, int n_groups, hipStream_t st);

// l2z_verify_tree (verify_tree.hip): the rows of a step are the nodes of a TREE of guesses on ONE sequence.  Node i stands
// for position pos0 + depth[i] (tab->pos[i]) and keeps its K / V in PHYSICAL cache row pos0 + i (tab->kc[i] / vc[i] are the
// cache bases shifted by (i - depth[i]) * head_size floats, so the step's epilogue stores there).  Uploaded behind the
// step's BatchTable in the same copy, where VerifyGroupTable sits for l2z_verify_batch.
struct VerifyTreeTable {
    int32_t parent[kBatchMax];  // parent[0] = -1, 0 <= parent[i] < i
    int32_t depth[kBatchMax];   // edges from node i to the root
    uint32_t below[kBatchMax];  // bit i of below[j]: node j lies on the path root -> i (j == i included)
    uint32_t level[kBatchMax];  // bit i of level[d]: depth[i] == d
};
static_assert(sizeof(BatchTable) % alignof(VerifyTreeTable) == 0, "the tree table sits right behind the step's table");
// Attention: block (head, segment) over kVerifySeg ABSOLUTE positions, the score buffer indexed by position as in
// launch_verify_attention.  Row i finds the key of position t in cache row t for t < pos0 and in row pos0 + (its ancestor
// of depth t - pos0) up to its own position; deeper positions are masked (weight exactly 0, V row skipped).  Every
// summation order is verify_device.h's, so row i's partials are the bits l2z_verify leaves for row depth[i] of the chain
// root -> i.  max_depth = the deepest node's depth; the grid is (n_heads, (pos0 + max_depth) / kVerifySeg + 1).
struct VerifyTreeAttnArgs : VerifyAttnArgs {
    const VerifyTreeTable *tree;
};
hipError_t launch_verify_tree_attention(const VerifyTreeAttnArgs &a, int n, int max_depth, hipStream_t st);
hipError_t launch_verify_tree_combine(const VerifyTreeAttnArgs &a, int n, int max_depth, hipStream_t st);
// The verdict: launch_verify_tree_accept walks the tree from the root over the rows' next ids out[0 .. n) -- while the node
// has a child whose token is the node's next id, go there -- and leaves out[n] = a (edges walked), out[n + 1 + d] = the node
// at depth d (d = 0 .. a), and the last node's row of the logits matrix in dst.
hipError_t launch_verify_tree_accept(const BatchTable *tab, const VerifyTreeTable *tree, const float *logits, int vocab, int *out,
                                     float *dst, int n, hipStream_t st);
// The accepted path's K / V rows into place, read from the verdict on the device (res = launch_verify_tree_accept's out):
// row pos0 + path[d] -> row pos0 + d for d = 1 .. a, every layer and kv head of both caches (kc / vc: layer 0's bases).
hipError_t launch_verify_tree_compact(float *kc, float *vc, const int *res, int n, int pos0, int head_size, size_t kv_head_stride,
                                      int n_layers, int n_kv_heads, hipStream_t st);

}  // namespace l2z
