/*
 * llama2_hip_test.h -- entry points of libllama2_hip.so that exist for TESTS and MEASUREMENT only.
 *
 * Nothing here is part of the drop-in boundary (include/llama2_hip.h): a host that replaces
 * src/main.zig's transformer() never calls these.  tests/, bench.py and scripts/ do:
 *   - kernel-level hooks named after the reference's math functions (src/main.zig:432-726), so the
 *     reference's own unit-test vectors (main.zig:1078-1150) can be run against the device code;
 *   - l2z_attention_decode: the decode attention kernels the forward pass launches, driven directly;
 *   - read-back of device state, the seeded synthetic-checkpoint generator, emulated ranks;
 *   - per-kernel timing and the streaming-read probe behind bench.py's roofline;
 *   - l2z_option_set: the tuning knobs of csrc/tunables.h from inside a process.
 */
#ifndef LLAMA2_HIP_TEST_H
#define LLAMA2_HIP_TEST_H

#include "llama2_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- synthetic checkpoints / state read-back ---- */
/* Same layout, filled ON DEVICE by the seeded generator of DESIGN.md
 * "Synthetic checkpoints" (no checkpoint exists in the build image, and a 27 GB
 * PCIe upload is not part of the measured path). */
int l2z_weights_init_synthetic(const l2z_config *config, int shared_weights, uint64_t seed,
                               const l2z_comm *comm, l2z_weights **out);
/* Copy `count` floats starting at index `offset` of the checkpoint's weight blob (FILE order, main.zig:85-112)
 * back to the host -- the device copy keeps W1 | W3 row-interleaved, this call undoes that
 * (single-GPU weights only; used by tests to check uploads / the generator). */
int l2z_weights_read(const l2z_weights *w, size_t offset, size_t count, float *out);

/* The 29-bit packed copy of each layer's W1 | W3 slot that the decode's ffn13 launch streams (csrc/packed_w.h,
 * DESIGN.md 4.9; unsharded weights, built at init unless L2Z_PACKED_W=0): how many layers' slots are packed, out of how
 * many of a width the packed kernel takes.  A slot with a NaN, an Inf, a denormal or a span of more than 31 binades
 * stays f32 only. */
int l2z_weights_packed_count(const l2z_weights *w, int *n_packed, int *n_candidates);
/* Decode the packed slot of `layer` ON THE DEVICE back to f32: 2 * hidden_dim rows (row 2r = W1 row r, row 2r + 1 = W3
 * row r) x dim, row-major, into out (n_floats >= that).  L2Z_ERR_STATE if that slot is not packed. */
int l2z_weights_packed_read(const l2z_weights *w, int layer, float *out, size_t n_floats);
/* The same two for the packed copy of any kind of decode launch (`kind`: the index l2z_time_kind takes).  Slots per layer:
 * qkv 3 (0 Wq, 1 Wk, 2 Wv: rows x dim each, every slot with its own base exponent; the launch streams the copy only if
 * all three of its layer are packed), wo 1 (dim x dim), ffn13 1 (the W1 | W3 slot above), ffn2 1 (dim x hidden_dim), cls
 * 1 for the model, at layer 0 (vocab_size x dim; with shared embeddings a copy of the embedding table).  A slot with an
 * odd number of rows is a candidate that stays f32.  Kinds without a packed form report (0, 0). */
int l2z_weights_packed_count_kind(const l2z_weights *w, int kind, int *n_packed, int *n_candidates);
int l2z_weights_packed_read_kind(const l2z_weights *w, int kind, int layer, int slot, float *out, size_t n_floats);
/* The bits a value that slot was packed at: 28 (rows of exactly 4096 values whose pairs have at most eight values below the
 * 4-bit exponent window, each carried in the pair's patch record; L2Z_PACKED_BITS=28, the default), 29, or 0 where the slot
 * has no packed copy.  The q|k|v slots of a layer report one form: 28 only if all three take it.  Both read calls above
 * decode either form. */
int l2z_weights_packed_bits_kind(const l2z_weights *w, int kind, int layer, int slot, int *bits);

/* copy a named RunState buffer to the host: "x","xb","hb","q","att","logits",
 * "key_cache","value_cache" (tests only) */
int l2z_runstate_read(l2z_runstate *s, const char *name, size_t offset, size_t count, float *out);


/* ---- measurement support ----
 * l2z_stream_read_probe streams `slice_bytes` pieces of the resident weight blob (0 = all of it)
 * through a pure read kernel `reps` times, a different piece per launch, and returns the average
 * and best read rate in GB/s: the measured ceiling bench.py quotes beside the 8 TB/s HBM3E spec
 * (SURVEY.md 8d "also report against a measured ... on the same box").
 * l2z_profile_forward runs ONE forward pass (+ argmax/hand-over) eagerly with
 * a HIP event pair around every kernel launch, recorded on the runstate's own
 * stream, and returns per-kind total device time (ms) and launch count.
 * Kinds, in slot order (l2z_kind_name): 0 "qkv", 1 "attn", 2 "wo", 3 "ffn13",
 * 4 "ffn2", 5 "cls", 6 "argmax" (0 launches when the classifier's last block hands the loop over
 * itself), 7 "gather" (sharded runs: gather launches); n_kinds must be >= 8.  bench.py derives the
 * roofline of the dominant kernel from this, in situ: every layer streams
 * its own weights, so nothing is re-read from cache between launches.  The
 * numbers must agree with rocprofv3 --kernel-trace --stats (profiles/). */
#define L2Z_N_KINDS 8
int l2z_stream_read_probe(l2z_runstate *s, const l2z_weights *w, size_t slice_bytes, int reps,
                          double *avg_gbps, double *best_gbps);
/* the same pieces copied device to device (hipMemcpyAsync) into a scratch allocation: GB/s of bytes COPIED
 * (memory traffic is twice that), SURVEY.md 8d's "measured device-to-device copy on the same box" */
int l2z_d2d_copy_probe(l2z_runstate *s, const l2z_weights *w, size_t slice_bytes, int reps,
                       double *avg_gbps, double *best_gbps);
int l2z_profile_forward(int token, int pos, const l2z_config *config, l2z_runstate *s,
                        const l2z_weights *w, double *ms_by_kind, int *launches_by_kind,
                        int n_kinds);
int l2z_kind_name(int kind, char *out, size_t cap);
/* Average duration of ONE launch of `kind` (0..6) at position `pos`: `reps` passes of that kind's
 * launches for every layer, back to back between ONE event pair on the runstate's stream -- no
 * per-launch event overhead, every launch streams its own layer's weights.  Comparable with
 * rocprofv3 --kernel-trace durations.  Unsharded runstates only. */
int l2z_time_kind(int kind, int pos, const l2z_config *config, l2z_runstate *s, const l2z_weights *w,
                  int reps, double *avg_ms_per_launch, int *launches);

/* ---- kernel-level test hooks (host pointers in and out; same device code
 *      the forward pass runs).  Names follow src/main.zig. ---- */
int l2z_matmul(float *xout, const float *x, const float *w, size_t n, size_t d);      /* :485 */
int l2z_matmul_fused(int N, float *const *outs, const float *x, const float *const *ws, size_t n,
                     size_t d);                                                        /* :530 */
int l2z_rmsnorm(float *o, const float *x, const float *w, size_t n);                   /* :432 */
int l2z_softmax(float *x, size_t n);                                                   /* :687 */
int l2z_vector_dot_product(float *out, const float *x, const float *y, size_t n);      /* :503 */
int l2z_vector_weighted_sum_rows(float *xout, size_t xout_len, const float *rows, size_t rows_len,
                                 size_t row_stride, const float *weights, size_t n_weights); /* :657 */
int l2z_argmax_host(const float *x, size_t n, size_t *out_index);                      /* :715 */

/* The decode attention of ONE layer (src/main.zig:361-389: scores :367-375, softmax :378 / :687-706,
 * weighted sum of V rows :381-388 / :657-685) through the kernels the forward pass launches.
 *   q [n_heads*head_size]; kcache, vcache [seq_len * kv_dim] (rows 0..pos are read);
 *   out [n_heads*head_size].   form: 0 = what the forward pass would pick at `pos`,
 *   1 = one block per head, 256 threads (speculative first round: seq_len <= 512 models),
 *   2 = one block per head, 1024 threads, 3 = split over `nch` blocks per head + combine
 *   (nch 0: the runstate default for n_heads), 4 = generic kernel. */
int l2z_attention_decode(int form, int nch, float *out, const float *q, const float *kcache,
                         const float *vcache, int pos, int n_heads, int n_kv_heads, int head_size,
                         int seq_len);

/* The batched prefill's attention kernels (llama2.zig_amd/csrc/prefill_attention.hip) for the n_queries
 * queries at positions pos0 .. pos0 + n_queries - 1 of one layer: q and out are [n_queries][n_heads * head_size],
 * the caches [seq_len][n_kv_heads * head_size] with rows 0 .. pos0 + n_queries - 1 filled.
 * form: 0 as l2z_prefill picks, 1 block per (head, query), 2 tiled with the softmax in LDS, 3 / 4 flash form
 * with one / two key parts (head sizes 64 and 128). */
int l2z_prefill_attention(int form, float *out, const float *q, const float *kcache, const float *vcache,
                          int pos0, int n_queries, int n_heads, int n_kv_heads, int head_size, int seq_len);

/* Host-side shard geometry (no device needed): out[0..9] = dim0, dim_loc, kvd_loc, heads_loc, hid0, hid_loc, v0, v_loc of
 * rank `rank` of `world` (scheme A: rows / heads owned), then dimc_pad, hidc_pad: the zero-padded row width of its Wo / W2
 * column shards under scheme B (multiples of 256 floats above 768, of 4 below).  L2Z_ERR_INVALID when the shape does not
 * split over `world` ranks. */
int l2z_shard_plan(const l2z_config *config, int rank, int world, int *out, int cap);

/* Host-side planning of the batched prefill (no device needed).  l2z_prefill_plan: the chunk lengths a
 * prompt of n_tokens is cut into (returns their number, writes up to cap of them).  l2z_prefill_tile: the
 * output tile of the direct-to-LDS GEMM for an [n_tokens, n_features] product -- 0: 128x64, 1: 64x64,
 * 2: 32x64, 3: 32x32, 4: 128x128 (all forms give the same bits; the choice fills the CUs). */
int l2z_prefill_plan(int n_tokens, int *chunks, int cap);
/* The same for a given model: where the model's matrices take the K-range panel kernel (chunks of 17 ... 64 tokens of
 * matrices that stream from HBM) a tail of 65 ... 96 tokens is cut in two chunks of that range (48 | 64 tokens first),
 * and a tail of 129 ... 160 / 257 ... 288 tokens into 128 / 256 + the rest. */
int l2z_prefill_plan_model(const l2z_config *config, int n_tokens, int *chunks, int cap);
int l2z_prefill_tile(int n_features, int n_tokens, int paired);
/* K ranges per output tile of the tile GEMM's split-K family for an [n_tokens, k] x [n_features_whole, k]^T
 * product (1: the unsplit family; > 1 also means the tile kernel instead of the short-prompt kernels).  Part of
 * the arithmetic -- the range partials are added in range order -- hence a function of the chunk length and the
 * WHOLE model's matrix, never of a rank's share of its rows. */
int l2z_prefill_split_k(long long n_features_whole, int n_tokens, int k, int paired);
/* The matrix cores of an [n_tokens, k] x [n_features_whole, k]^T product (round 6): 0 the f32 ones
 * (v_mfma_f32_32x32x2_f32, an fmaf chain), 1 the bf16 ones over three-term splits of both operands (six
 * v_mfma_f32_32x32x16_bf16 per 16 k; matrices that stream from HBM, or all with L2Z_PF_X3=2) in the tile forms, n >= 2: the
 * STREAM form of that kernel (chunks of L2Z_PF_X3_STREAM_MIN = 33 ... 128 tokens) with n - 1 K ranges per output tile -- part of
 * the arithmetic, a function of the chunk length and the WHOLE model's matrix.  k: the product's K (rounded up to 64 here). */
int l2z_prefill_cores(long long n_features_whole, int n_tokens, int k);
/* Which kernel a product of the batched prefill takes, and in which form (host logic; the CU count is the current device's,
 * 256 without one).  shape: kind 0 one matrix (epi: 0 store, 1 residual, 2 RoPE, 3 RoPE into the key cache, 4 into the value
 * cache, 5 SwiGLU merge), 1 q | k | v fused (n_features = nq + 2 nkv), 2 W1 | W3 paired (n_features of each; w13_one_matrix:
 * their rows alternate in one slot), 3 k | v paired; n_features / nq / nkv are THIS rank's rows of n_scale ranks;
 * n_launch_whole: rows of the whole model's launch the product is a part of (0: n_features * n_scale); sk: l2z_prefill_split_k
 * of the whole product; part_floats, cnt_ints: the split workspace.  plan: family 1 stream, 2 short-prompt (tms token tiles
 * of 16 per block, paired), 3 split-K, 4 k-groups on two blocks, 5 tile; -1 invalid, -2 not supported (launch the products
 * apart), -3 the workspace is too small.  epi: the kernel's epilogue (6 q | k | v, 7 W1 | W3 interleaved); k: K as the kernel
 * walks it; x3: on the bf16 cores; sk: K ranges per tile; tile: as l2z_prefill_tile; stream form: feat features per block, tm
 * token tiles of 32, ring depth nbuf, one_round: one block per CU. */
typedef struct { int kind, epi, n_tokens, n_features, k, ldx, n_scale, sk, nq, nkv, w13_one_matrix, cnt_ints;
                 long long n_launch_whole, part_floats; } l2z_gemm_shape;
typedef struct { int family, epi, k, x3, sk, tile, feat, tm, nbuf, one_round, tms, paired; } l2z_gemm_plan;
int l2z_prefill_gemm_plan(const l2z_gemm_shape *shape, l2z_gemm_plan *plan);

/* ---- emulated ranks ---- */
/* Testing support: N emulated ranks in ONE process on ONE GPU (RCCL refuses two ranks on
 * one device).  l2z_comm_init_emulated makes a rank descriptor without a communicator;
 * weights / runstates built with it hold exactly rank r's shard; l2z_emu_transformer runs
 * one forward pass for all ranks, interleaved stage by stage, doing each all-gather as
 * device-to-device copies.  Afterwards every rank's logits must equal the unsharded pass. */
int l2z_comm_init_emulated(int rank, int world, int device, l2z_comm **out);
int l2z_emu_transformer(int n_ranks, l2z_runstate *const *ss, const l2z_weights *const *ws,
                        int token, int pos);
/* l2z_prefill for the emulated ranks: every rank's own launches of each stage (llama2.zig_amd/csrc/
 * prefill_host.cpp), the [tokens, n / world] activation blocks exchanged as device-to-device copies.
 * Afterwards every rank's KV shard and logits must equal the unsharded l2z_prefill, bit for bit. */
int l2z_emu_prefill(int n_ranks, l2z_runstate *const *ss, const l2z_weights *const *ws,
                    const int32_t *tokens, int n_tokens, int pos0);

/* What a shard group's transports are (bench.py's comm{} record): the rank count RCCL itself reports
 * for the communicator (ncclCommCount; 0 when the group has none) and whether the peer-write arenas
 * are connected. */
int l2z_comm_transports(const l2z_comm *c, int *rccl_ranks, int *p2p_connected);

/* Measurement: after l2z_comm_p2p_export, connect this rank ALONE -- every peer's arena is a local sink, this rank's own zeroed slots satisfy every hand-over's
 * wait is satisfied by the zeroed slots -- so that ONE rank of an N-rank group runs its whole sharded pass (launches,
 * pushes, polls, gather / reduce launches) on a GPU by itself: the per-rank time with free hand-overs.  Results are
 * meaningless (the peers' slices read as zeros). */
int l2z_comm_p2p_connect_solo(l2z_comm *c);

/* Diagnostics of the peer-write transport, for bench.py's N > 1 legs (what a hand-over costs between two ranks of
 * THIS group on THIS box -- xGMI when they sit on two GPUs).  Both are made by two ranks at once, like every call of a
 * shard group: l2z_comm_p2p_pingpong by `other` and by this rank with opposite `initiator` flags and the same iters --
 * *rtt_us = microseconds per round trip of one 8-byte LL word each way (device clock, one polling thread per side);
 * l2z_comm_peer_copy_probe by one rank only: `bytes` into the other's arena by the runtime's device-to-device copy,
 * each copy synchronised: microseconds per copy (host clock). */
int l2z_comm_p2p_pingpong(l2z_comm *c, int other, int initiator, int iters, double *rtt_us);
int l2z_comm_peer_copy_probe(l2z_comm *c, int other, size_t bytes, int iters, double *us_per_copy);

/* Loads RCCL (dlopen) now and reports the file the process got and ncclGetVersion's code.  A process that imports
 * PyTorch afterwards keeps THIS copy (same SONAME); one that imported it before gets torch's bundled copy. */
int l2z_comm_rccl_info(char *path_out, size_t cap, int *version);

/* The structure a runstate runs: bit 3 = sharding scheme B (L2Z_SCHEME_B: column-sharded Wo / W2 + all-reduces);
 * 0 = the default.  (Bits 0-2 named round 4's opt-in decode forms, removed in round 5: always 0.)  Tests that ask
 * for an option check here that they got it. */
int l2z_runstate_form(const l2z_runstate *s, int *form);

/* Set one tuning knob by its environment-variable name (csrc/tunables.h), e.g. ("L2Z_P2P_CONSUME", 0).
 * Applies to objects created afterwards.  L2Z_ERR_INVALID for an unknown name. */
int l2z_option_set(const char *env_name, long long value);

/* Measurement (scripts/batch_bench.py): one l2z_transformer_batch call, then `iters` more back to back, timed by device
 * events on the pass's stream; *out_ms = milliseconds per step.  The steps rewrite the same KV rows. */
int l2z_batch_time(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                   l2z_runstate *const *states, const l2z_weights *w, int iters, double *out_ms);
/* Place exact logits (vocab_size floats) in an unsharded runstate: the distributions l2z_sample_batch is tested on
 * (ties at the top-p cut, peaked, uniform, one-hot).  Synchronous. */
int l2z_logits_write(l2z_runstate *s, const float *logits);
/* Measurement (scripts/sample_bench.py): one l2z_sample_batch launch, then `iters` more back to back without the copy
 * back, timed by device events on states[0]'s stream; *out_ms = milliseconds per launch. */
int l2z_sample_time(int n, l2z_runstate *const *states, const float *temperature, const float *top_p,
                    const float *coins, int iters, double *out_ms);
/* l2z_score's classifier product on this runstate goes out in slabs of `slab_cols` vocabulary rows: a positive multiple
 * of 4096 (the reduction's segment; else L2Z_ERR_INVALID), or 0 for the default (by the workspace budget).  Applies from
 * the next l2z_score call.  The outputs do not depend on it, bit for bit: that is what the tests use it for. */
int l2z_score_slab_set(l2z_runstate *s, int slab_cols);
/* Row `row` (0 .. n_tokens - 1) of the logits matrix of this runstate's last l2z_verify or l2z_verify_sample call: every z_i, not only the
 * accepted z_a the runstate keeps (vocab_size floats).  L2Z_ERR_STATE when there is no such row.  Synchronous.  After
 * l2z_verify_batch and l2z_verify_wide the matrix is states[0]'s: row r of the concatenated rows; the call's other runstates
 * have no row. */
int l2z_verify_logits_read(l2z_runstate *s, int row, float *out);
/* Measurement (scripts/verify_bench.py): one l2z_verify call, then `iters` passes back to back (verdict launches and
 * their copy included, no sync), timed by device events on the runstate's stream; *out_ms = milliseconds per pass.  The
 * passes rewrite the same KV rows.  The twin of l2z_batch_time. */
int l2z_verify_time(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
                    const l2z_weights *w, int iters, double *out_ms);
/* Measurement (scripts/verify_sample_bench.py): the twin of l2z_verify_time for l2z_verify_sample -- one call, then `iters`
 * passes back to back (the rows' draws, the accept scan and the copy included, no sync); *out_ms = milliseconds per pass. */
int l2z_verify_sample_time(const int32_t *tokens, int n_tokens, int pos0, float temperature, float top_p,
                           const float *coins, const l2z_config *config, l2z_runstate *s, const l2z_weights *w, int iters,
                           double *out_ms);

/* ---- preview entry points ----
 * Public through the Python binding, exported by libllama2_hip_test.so only: not part of ABI version 2 (include/llama2_hip.h
 * and its 31 functions are unchanged).  Promotion into the product header, the Zig shim and the CLI (llama2 -b N with one
 * prompt per line) belongs to the change that cuts ABI version 3. */

/* Ragged batched prefill: the prompts of n sequences, one runstate each, in ONE pass -- every weight matrix streamed once per
 * chunk of the concatenated rows instead of once per sequence (what l2z_transformer_batch is to l2z_transformer, for
 * l2z_prefill).  Sequence j contributes n_tokens[j] consecutive positions starting at pos0[j]; tokens = the sequences'
 * tokens concatenated in order (the sum of n_tokens[] entries).
 * For every j the call leaves the state l2z_prefill(tokens_j, n_tokens[j], pos0[j], config, states[j], w) leaves: KV rows
 * pos0[j] .. pos0[j] + n_tokens[j] - 1 of every layer of states[j] written -- and NO other cache row of any runstate --
 * and states[j]'s logits those of its last position, so l2z_argmax, l2z_logits_read, l2z_probs_read, l2z_sample_batch,
 * l2z_transformer_batch, l2z_verify and l2z_runstate_fork go on from there.  Values agree with l2z_prefill's up to summation
 * order (the fp32 parity bar), not bit for bit: the GEMM form follows the chunk's TOTAL row count and the attention kernel
 * is another one.
 * The concatenated rows are cut into chunks by l2z_prefill's plan applied to the total (L2Z_PF_CHUNK as there); a sequence
 * may straddle a chunk boundary, and pos0[j] > 0 continues a sequence (after l2z_runstate_fork, or an earlier call).
 * Neighbour invariance: for a fixed layout -- the same n, n_tokens[], pos0[], order and chunking -- sequence j's KV rows
 * and logits are bit-identical whatever tokens the other sequences hold and whatever their caches contain, and from run to
 * run.  Nothing more is promised: the other sequences' LENGTHS matter, because the total row count selects the kernel form.
 * The prefill scratch is states[0]'s (freed with it).  The pass runs on states[0]'s stream after everything queued on every
 * runstate's stream, and every runstate's stream waits for it (l2z_transformer_batch's rule; no device-wide sync); like
 * l2z_prefill the call returns once its work has completed.
 * A refusal enqueues nothing and changes no state.  L2Z_ERR_INVALID: a NULL argument, n outside [1, L2Z_BATCH_MAX], an
 * n_tokens[j] < 1, runstates that are not pairwise distinct, unsharded, on one device and made with *config, weights of
 * another config, dims l2z_prefill refuses.  L2Z_ERR_STATE: pos0[j] < 0, pos0[j] + n_tokens[j] > seq_len, a token outside
 * the vocabulary.  L2Z_ERR_NO_DEVICE without a device. */
int l2z_prefill_batch(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                      const l2z_config *config, l2z_runstate *const *states, const l2z_weights *w);

/* Batched speculative decoding: the verify pass of l2z_verify / l2z_verify_sample for n sequences, one runstate each, in ONE
 * sweep of the weights.  Sequence j contributes n_tokens[j] consecutive positions from pos0[j]: its first token is known, the
 * rest are guesses.  tokens, coins and out_next are the sequences' rows concatenated in order: R = the sum of n_tokens[] rows,
 * R <= L2Z_BATCH_MAX; out_accepted has n entries.
 * temperature == NULL: every sequence is greedy; top_p and coins are ignored and may be NULL.  Otherwise temperature[j] and
 * top_p[j] are per sequence and coins is per row; a sequence with temperature[j] == 0 is arg-maxed (its coins are not read).
 * THE DEFINING PROPERTY: for every j the outputs and the state left in states[j] are bit-identical to what the
 * single-sequence call leaves on the same state -- l2z_verify(tokens_j, n_tokens[j], pos0[j], config, states[j], w, ...), or
 * l2z_verify_sample with temperature[j], top_p[j] and coins_j -- whatever n is, whatever the other sequences hold, and in any
 * order of the sequences within the call.  Outputs and state: out_next_j and out_accepted[j]; KV rows pos0[j] ..
 * pos0[j] + n_tokens[j] - 1 of every layer; the runstate's logits (z_a); the next position pos0[j] + a_j + 1.  (DRAFT
 * INVARIANCE and BATCH INVARIANCE of include/llama2_hip.h, extended: the products take one kernel form whatever the row count,
 * and the attention's orders depend on head_size, the segment and the row's position alone.)  No cache row outside a
 * sequence's own pos0[j] .. pos0[j] + n_tokens[j] - 1 is written, in any runstate.
 * With one row per sequence the call is a batched decode step on the position-split attention; its bits are l2z_verify's,
 * not l2z_transformer_batch's.
 * The pass runs on states[0]'s stream after everything queued on every runstate's stream, and every runstate's stream waits
 * for it (l2z_transformer_batch's rule); the scratch is states[0]'s; the call is synchronous as l2z_verify is (one copy back,
 * one sync).  Afterwards l2z_verify_logits_read(states[0], r, ...) returns concatenated row r; on states[j], j > 0, it
 * refuses with L2Z_ERR_STATE until that runstate's next call of its own.
 * A refusal enqueues nothing and changes no state.  L2Z_ERR_INVALID: a NULL required argument, n outside [1, L2Z_BATCH_MAX],
 * an n_tokens[j] < 1, R > L2Z_BATCH_MAX, runstates that are not pairwise distinct, unsharded, on one device and made with
 * *config, weights of another config, dims l2z_verify refuses, a temperature[j] that is not finite and >= 0, a top_p[j]
 * outside [0, 1] (or top_p == NULL beside temperature), coins == NULL with any temperature[j] > 0, a coin of such a sequence
 * outside [0, 1).  L2Z_ERR_STATE: pos0[j] < 0, pos0[j] + n_tokens[j] > seq_len, a token outside the vocabulary.
 * L2Z_ERR_NO_DEVICE without a device. */
int l2z_verify_batch(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                     const float *temperature, const float *top_p, const float *coins,
                     const l2z_config *config, l2z_runstate *const *states, const l2z_weights *w,
                     int32_t *out_next, int32_t *out_accepted);

/* Tree speculation: the verify pass of l2z_verify / l2z_verify_sample for a TREE of guesses on one sequence, in ONE sweep of
 * the weights -- several candidate continuations cost what one chain of as many rows costs.
 * Node 0 is the sequence's known token at pos0, parent[0] == -1.  Node i > 0 is a guess with 0 <= parent[i] < i (topological
 * order); depth_i = the number of edges from node i to the root, and node i stands for position pos0 + depth_i.
 * 1 <= n_nodes <= L2Z_BATCH_MAX; siblings carry pairwise different tokens.  A chain (parent[i] == i - 1) is l2z_verify's call.
 * Row i: z_i = the logits of position pos0 + depth_i given the tokens on the path root -> i on top of cache rows < pos0.
 * out_next[i] = the argmax of z_i (l2z_argmax's tie rule) at temperature == 0, otherwise the token l2z_sample_batch's kernel
 * draws from z_i with (temperature, top_p, coins[depth_i]): coins has one entry per DEPTH, coins[d] = the coin of position
 * pos0 + d, shared by all nodes of that depth; it may be NULL at temperature 0.
 * The verdict (on the device): cur = 0; while cur has a child c with tokens[c] == out_next[cur], cur = c.
 * out_path[0 .. a] = the nodes walked (out_path[0] == 0), *out_accepted = a; the sequence's next a + 1 tokens are
 * out_next[out_path[d]], d = 0 .. a.  out_path has room for n_nodes entries.
 * State on return (the shape of l2z_verify's): KV rows pos0 .. pos0 + a of every layer are the accepted path's, the runstate's
 * logits are z of node out_path[a], the next position is pos0 + a + 1.  During the pass node i's keys and values sit in cache
 * row pos0 + i; the accepted ones are moved into place on the device.  Rows pos0 + a + 1 .. pos0 + n_nodes - 1 hold rejected
 * nodes' rows: beyond the next position, which every entry point overwrites before it reads.  No row < pos0 and no row
 * >= pos0 + n_nodes is touched.  The call is synchronous; l2z_verify_logits_read(s, i, ...) returns z_i afterwards.
 * PATH INVARIANCE: z_i, node i's K / V rows and -- after the call -- cache rows pos0 .. pos0 + a and the runstate's logits
 * equal, BIT FOR BIT, what l2z_verify computes at row depth_i when it is given the tokens on the path root -> i as a chain on
 * the same cache rows < pos0.  They do not depend on the other branches, on n_nodes or on the numbering of the nodes.  So a
 * greedy loop over this call emits the ids of the loop over l2z_verify whatever the drafter proposes, and a sampled loop the
 * ids of the loop over l2z_verify_sample for the same coin sequence: the token of a position is drawn from that position's
 * distribution with that position's coin whatever the tree looks like, so the text keeps the plain sampler's law.
 * A refusal enqueues nothing and changes no state.  L2Z_ERR_INVALID: a NULL argument, n_nodes outside [1, L2Z_BATCH_MAX],
 * parent[0] != -1, a parent[i] outside [0, i), two siblings with one token, a sharded runstate, dims l2z_transformer_batch
 * refuses, l2z_verify_sample's rules for temperature / top_p / coins applied to coins[0 .. max depth].  L2Z_ERR_STATE:
 * pos0 < 0, pos0 + n_nodes > seq_len, a token outside the vocabulary.  L2Z_ERR_NO_DEVICE without a device. */
int l2z_verify_tree(const int32_t *tokens, const int32_t *parent, int n_nodes, int pos0,
                    float temperature, float top_p, const float *coins,
                    const l2z_config *config, l2z_runstate *s, const l2z_weights *w,
                    int32_t *out_next, int32_t *out_path, int *out_accepted);
/* Measurement (scripts/verify_tree_bench.py): the twin of l2z_verify_time for l2z_verify_tree -- one call, then `iters` passes
 * back to back (verdict, compaction and the copy included, no sync); *out_ms = milliseconds per pass. */
int l2z_verify_tree_time(const int32_t *tokens, const int32_t *parent, int n_nodes, int pos0,
                         float temperature, float top_p, const float *coins,
                         const l2z_config *config, l2z_runstate *s, const l2z_weights *w, int iters, double *out_ms);

/* The sampled generation loop on the device: l2z_greedy_run with the argmax replaced by the sampler's draw -- main.zig:987-1042
 * at any temperature, one replay of a captured step graph per position (forward pass, draw, prompt override, hand-over of
 * token and position, embedding row of the next token), no host round trip per token.
 * It follows l2z_greedy_begin (there is no second "begin") and shares the greedy loop's state -- the prompt, the ids, the next
 * position, the BOS flag -- so a sequence may alternate l2z_greedy_run and l2z_sample_run calls, and temperature and top_p may
 * change from call to call.
 * Step i of the call is position next + i.  Below the prompt's length the next token is prompt[pos] (main.zig:999-1000) and
 * coins[i] is not used; otherwise it is the token l2z_sample_batch draws from that step's logits with (temperature, top_p,
 * coins[i]) -- the same device code, so the same bits.  temperature == 0 takes the argmax (l2z_argmax's rule) and coins may be
 * NULL.  coins holds n_steps entries.
 * The call stops after a BOS and at seq_len, as l2z_greedy_run does: the host looks for BOS once per chunk of 64 steps (the
 * chunk's steps behind a BOS have run and are discarded), *out_n counts up to and including the BOS, and further calls return
 * 0 tokens until the next l2z_greedy_begin.  The prompt positions run as one batched pass under exactly l2z_greedy_run's
 * conditions.  The logits are not modified: l2z_logits_read afterwards returns the last step's.
 * The scratch (5 x vocab_size floats, one l2z_sample_batch row's) and one coin slot per position are allocated on the
 * runstate's first call and freed with it; the sampled step's graphs are captured on first use, so a runstate that only ever
 * runs greedy pays nothing.
 * A refusal enqueues nothing and changes no state.  L2Z_ERR_INVALID: a NULL argument, n_steps < 0, a sharded runstate,
 * l2z_greedy_run's refusals (config / runstate / weights that do not belong together), a temperature that is not finite and
 * >= 0, a top_p outside [0, 1], coins == NULL with temperature > 0, a coins[i] outside [0, 1) (NaN included; all n_steps
 * entries are checked, at temperature > 0).  L2Z_ERR_NO_DEVICE without a device.
 * Out of scope: sharded runstates (a shard's logits are its own vocabulary rows only), several sequences per call
 * (l2z_transformer_batch + l2z_sample_batch), and the CLI, which links the product library. */
int l2z_sample_run(const l2z_config *config, l2z_runstate *s, const l2z_weights *w, int n_steps,
                   float temperature, float top_p, const float *coins,
                   int32_t *out_tokens, int *out_n);

/* ---- wide batched decode (preview) ----
 * One decode step for up to L2Z_WIDE_MAX independent sequences, one runstate each, with one sweep of the weights on the
 * matrix cores: the n rows are ONE chunk of n rows of the ragged prompt pass (l2z_prefill_batch's) on states[0]'s prefill
 * scratch, so every product takes the whole model's GEMM form at that row count, and the attention is a position-split
 * decode kernel in which a block reads a kv head's K / V rows of one segment once for all the query heads that share them.
 * The state change is l2z_transformer_batch's, for 1 <= n <= L2Z_WIDE_MAX: KV row pos[i] of every layer of states[i] is
 * written -- and NO other cache row of any runstate --, states[i]'s logits hold its result, and every runstate's host
 * bookkeeping is left as l2z_transformer_batch leaves it (next position pos[i] + 1, whole logits, no per-block argmax
 * candidates): l2z_argmax, l2z_logits_read, l2z_probs_read, l2z_sample_batch, l2z_transformer_batch, l2z_verify* and
 * l2z_runstate_fork go on from there.
 * out_next != NULL: out_next[i] = the argmax of row i by l2z_argmax's rule (strict '>', the lowest index wins), taken on
 * the device by the launch that hands out the logits; the call returns after one copy and one sync.  out_next == NULL: the
 * call is asynchronous, as l2z_transformer_batch is.
 * Streams: l2z_transformer_batch's rule -- the pass runs on states[0]'s stream after everything queued on every runstate's
 * stream, and every runstate's stream waits for it; no device-wide sync.  The scratch is states[0]'s (freed with it).
 * INVARIANCE.  For a fixed n and a fixed place i in the batch, row i's logits and KV row are bit-identical whatever the
 * other rows' tokens, positions and caches hold and whatever stale rows lie beyond pos[i] in its own cache, and from run
 * to run: the GEMMs compute each row from that row alone in an order fixed by the shape and n, no block of the step's own
 * kernels touches two sequences, and the attention's orders depend on head_size, the segment and the row's own position
 * only.  Nothing more is promised: n selects the GEMM form, so values across different n, and against
 * l2z_transformer_batch / l2z_transformer, agree at the fp32 parity bar, not bit for bit.  l2z_transformer_batch stays the
 * form for n <= L2Z_BATCH_MAX whenever bit-invariance across n matters.
 * The step itself draws nothing but the argmax: draw with l2z_sample_batch in groups of L2Z_BATCH_MAX runstates after the
 * call, or run the steps and their draws on the device with l2z_wide_run (below).
 * A refusal enqueues nothing and changes no state.  L2Z_ERR_INVALID: a NULL argument other than out_next, n outside
 * [1, L2Z_WIDE_MAX], runstates that are not pairwise distinct, unsharded, on one device and made with *config, weights of
 * another config, dims l2z_prefill refuses.  L2Z_ERR_STATE: a pos[i] outside [0, seq_len), a token outside the vocabulary.
 * L2Z_ERR_NO_DEVICE without a device. */
#define L2Z_WIDE_MAX 128
int l2z_transformer_wide(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                         l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next /* may be NULL */);

/* ---- wide generation loop on the device (preview) ----
 * n_steps consecutive l2z_transformer_wide steps of the same n runstates in ONE call, every row's token drawn on the
 * device and handed to the next step there.  Step k (k = 0 .. n_steps - 1) runs transformer(tok_k[i], pos0[i] + k) on
 * states[i] exactly as l2z_transformer_wide runs it at that n; tok_0 = first_tokens, tok_{k+1}[i] = out_tokens[k * n + i],
 * and out_tokens[k * n + i] is the token l2z_sample_batch draws from that row's logits with (temperature[i], top_p[i],
 * coins[k * n + i]) -- the same device code, so the host samplers' bits.  Where temperature[i] == 0, or temperature ==
 * NULL (every row greedy; top_p and coins are not read), it is the argmax by l2z_argmax's rule and the coin is not read.
 * THE DEFINING PROPERTY: the ids, every row's final logits and every cache row are bit-identical to the step loop on the
 * same states -- l2z_transformer_wide(n, tok_k, pos0 + k, ..., NULL), then l2z_sample_batch over the runstates in groups
 * of L2Z_BATCH_MAX, for each k: the run issues each step's own launches, its attention grid sized by that step's own
 * deepest position.
 * On return KV rows pos0[i] .. pos0[i] + n_steps - 1 of every layer of states[i] are written -- and NO other cache row of
 * any runstate --, states[i]'s logits are its last step's, and the host bookkeeping is as l2z_transformer_wide leaves it
 * after the last step (next position pos0[i] + n_steps, whole logits, no per-block argmax candidates): every other entry
 * point can go on from there.
 * Nothing stops a row on the device: a row that draws BOS keeps running and the caller discards what follows it, as
 * l2z_sample_run's caller does within a chunk; the context limit is the caller's to keep (below).
 * The call is synchronous: the run waits for every runstate's stream once at its start, every runstate's stream waits
 * for it once at its end, and the call returns after one copy of the ids and one sync; no device-wide sync.  The scratch
 * is states[0]'s (freed with it); the sampler's (5 * vocab floats for each of L2Z_WIDE_MAX rows) is allocated on the
 * first call with a positive temperature -- runs that are all greedy allocate none.
 * A refusal enqueues nothing and changes no state.  L2Z_ERR_INVALID: everything l2z_transformer_wide refuses so,
 * n_steps < 1, NULL first_tokens, pos0 or out_tokens, a temperature that is not finite and >= 0, a top_p outside [0, 1]
 * or top_p == NULL beside temperature, coins == NULL with any temperature[i] > 0, a coin of such a row (all n_steps of
 * them) outside [0, 1).  L2Z_ERR_STATE: a pos0[i] < 0 or pos0[i] + n_steps > seq_len, a first token outside the
 * vocabulary.  L2Z_ERR_NO_DEVICE without a device. */
int l2z_wide_run(int n, const int32_t *first_tokens, const int32_t *pos0, int n_steps,
                 const float *temperature /* [n], or NULL: all greedy */, const float *top_p /* [n] */,
                 const float *coins /* [n_steps, n], row-major by step */,
                 const l2z_config *config, l2z_runstate *const *states, const l2z_weights *w,
                 int32_t *out_tokens /* [n_steps, n] */);

/* ---- wide speculative decoding (preview) ----
 * The verify pass of l2z_verify_batch for up to L2Z_WIDE_MAX rows in ONE sweep of the weights on the matrix cores: the rows
 * are one chunk of R rows of the ragged prompt pass on states[0]'s prefill scratch, as l2z_transformer_wide's are, with
 * several rows per sequence.  The arguments have l2z_verify_batch's meaning throughout: sequence j contributes n_tokens[j]
 * consecutive positions from pos0[j], its first token known and the rest guesses; tokens, coins and out_next are the
 * sequences' rows concatenated in order; temperature and top_p are per sequence (temperature == NULL: every sequence greedy,
 * top_p and coins not read; a sequence at temperature 0 is arg-maxed and its coins are not read); out_accepted has n entries.
 * 1 <= n <= L2Z_WIDE_MAX, 1 <= n_tokens[j] <= L2Z_BATCH_MAX, R = the sum of n_tokens[] <= L2Z_WIDE_MAX.
 * Row r: z_r = the logits of its position given its sequence's tokens up to it on top of cache rows < pos0[j]; out_next[r] =
 * the argmax of z_r, or the sampler's draw; out_accepted[j] = a_j, the number of leading guesses that equal the row before's
 * out_next (found on the device).  State on return, per sequence, l2z_verify's: KV rows pos0[j] .. pos0[j] + n_tokens[j] - 1
 * of every layer written -- and NO other cache row of any runstate --, the runstate's logits z_a, the next position
 * pos0[j] + a_j + 1, and the host bookkeeping as l2z_transformer_wide leaves it (whole logits, no per-block argmax
 * candidates): every other entry point goes on from there.
 * The call is synchronous (one copy back, one sync).  Streams: l2z_transformer_batch's rule.  The scratch is states[0]'s wide
 * scratch (freed with it); the sampler's is allocated on the first call with a positive temperature.  Afterwards
 * l2z_verify_logits_read(states[0], r, ...) returns concatenated row r, r < R; on the call's other runstates it refuses with
 * L2Z_ERR_STATE until that runstate's next verify call of its own.
 * WHAT IS PROMISED.  The products take the whole model's GEMM form at R rows, so a row's bits depend on the total row count
 * and possibly on the row's place: this call does NOT inherit the bit-for-bit DRAFT INVARIANCE across calls that l2z_verify,
 * l2z_verify_sample, l2z_verify_batch and l2z_verify_tree have.  It promises:
 *   ONE-ROW IDENTITY.  With every n_tokens[j] == 1 and all greedy, each runstate's logits, every cache row and out_next are
 *     bit-identical to l2z_transformer_wide on the same states, tokens, positions and order: the same chunk of the same R
 *     rows, and a slot's bits in the segment attention do not depend on how many slots a block has or on what a slot is.
 *   NEIGHBOUR INVARIANCE.  For a fixed layout -- the same n, n_tokens[], pos0[] and order -- sequence j's out_next,
 *     out_accepted[j], logits and KV rows are bit-identical whatever the other sequences' tokens and caches hold, whatever
 *     stale rows lie beyond its own rows, and from run to run.
 *   CAUSALITY within a call.  Row i of a sequence is a function of that sequence's tokens 0 .. i and the cache rows below
 *     pos0 alone: changing the guesses behind row i leaves logits row i and KV row pos0 + i bit-identical.
 *   PARITY.  Values against l2z_verify / l2z_verify_batch, and against the CPU oracle, agree at the fp32 parity bar, not bit
 *     for bit.
 *   THE DRAW.  Given row r's logits, out_next[r] is bit for bit the token l2z_sample_batch draws from them with the same
 *     temperature, top_p and coin (the argmax by l2z_argmax's rule at temperature 0).
 * l2z_verify_batch stays the form for R <= L2Z_BATCH_MAX and wherever the text must not depend on the drafter bit for bit.
 * A refusal enqueues nothing and changes no state.  L2Z_ERR_INVALID: a NULL required argument, n outside [1, L2Z_WIDE_MAX],
 * an n_tokens[j] outside [1, L2Z_BATCH_MAX], R > L2Z_WIDE_MAX, runstates that are not pairwise distinct, unsharded, on one
 * device and made with *config, weights of another config, dims l2z_prefill refuses, a temperature[j] that is not finite and
 * >= 0, a top_p[j] outside [0, 1] (or top_p == NULL beside temperature), coins == NULL with any temperature[j] > 0, a coin
 * of such a sequence outside [0, 1).  L2Z_ERR_STATE: pos0[j] < 0, pos0[j] + n_tokens[j] > seq_len, a token outside the
 * vocabulary.  L2Z_ERR_NO_DEVICE without a device.
 * Out of scope: the product header, map, Zig shim and CLI (ABI version 3); sharded runstates; trees; the loop on the
 * device; sharing a kv head's K / V rows between its query heads in the multi-row attention; hipGraph replay. */
int l2z_verify_wide(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                    const float *temperature, const float *top_p, const float *coins,
                    const l2z_config *config, l2z_runstate *const *states, const l2z_weights *w,
                    int32_t *out_next, int32_t *out_accepted);

/* ---- mixed step: prompt chunks and decode rows in one sweep of the weights (preview) ----
 * What a server does when a request arrives while others decode: n sequences, one runstate each, of which sequence j brings
 * n_tokens[j] consecutive positions pos0[j] .. pos0[j] + n_tokens[j] - 1.  A sequence of ONE row is a decode step; a sequence
 * of two or more rows is a prompt chunk -- a whole prompt, or a slice of one that starts at pos0[j] > 0 (chunked prefill).
 * tokens is the sequences' rows concatenated.  1 <= n <= L2Z_WIDE_MAX, n_tokens[j] >= 1, R = the sum of n_tokens[] <=
 * L2Z_MIXED_ROWS_MAX.  The R rows run as ONE chunk of the ragged prompt pass on states[0]'s prefill scratch, as
 * l2z_transformer_wide's n rows do: every weight matrix is read once per call.  Per layer the multi-row sequences take the
 * prompt attention of l2z_prefill_batch, the one-row sequences the position-split decode attention of l2z_transformer_wide;
 * the classifier runs on the n LAST rows only.
 * State on return, per sequence: KV rows pos0[j] .. pos0[j] + n_tokens[j] - 1 of every layer written -- and NO other cache
 * row of any runstate --, the runstate's logits those of its last row, the next position pos0[j] + n_tokens[j], the host
 * bookkeeping as l2z_transformer_wide leaves it (whole logits, no per-block argmax candidates): every other entry point goes
 * on from there.  out_next[j] = the token the sampler draws from those logits with (temperature[j], top_p[j], coins[j]) --
 * ONE coin per sequence --; at temperature 0, or temperature == NULL (top_p and coins not read), the argmax by l2z_argmax's
 * rule.  A caller in the middle of a prompt ignores the id.
 * The call is synchronous (one copy back, one sync).  Streams: l2z_transformer_batch's rule.  Paged runstates are taken as
 * the wide family takes them (all of one kind; pages attached on the host before anything is enqueued; L2Z_ERR_OOM leaves
 * nothing attached; a write into a shared page is L2Z_ERR_STATE).
 * WHAT IS PROMISED.
 *   ALL-ONE-ROW IDENTITY.  With every n_tokens[j] == 1, each runstate's logits and every cache row are bit-identical to
 *     l2z_transformer_wide on the same states, tokens, positions and order.
 *   PROMPTS-ONLY IDENTITY.  With n <= L2Z_BATCH_MAX and every n_tokens[j] >= 2, every cache row is bit-identical to
 *     l2z_prefill_batch on the same layout (while that call runs it as one chunk); the logits agree at the parity bar (that
 *     call takes them by the mat-vec classifier).
 *   NEIGHBOUR INVARIANCE.  For a fixed layout, sequence j's id, logits and KV rows are bit-identical whatever the other
 *     sequences' tokens and caches hold, whatever stale rows lie beyond its own, and from run to run.
 *   THE DRAW.  Given a sequence's logits, out_next[j] is bit for bit l2z_sample_batch's token for the same controls.
 *   PARITY.  Against the CPU oracle and against l2z_prefill_batch followed by l2z_transformer_wide: the fp32 parity bar.
 *   PAGED == contiguous, bit for bit.
 * A refusal enqueues nothing and changes no state.  L2Z_ERR_INVALID: a NULL required argument, n outside [1, L2Z_WIDE_MAX],
 * an n_tokens[j] < 1, R > L2Z_MIXED_ROWS_MAX, runstates that are not pairwise distinct, unsharded, of one kind, on one device
 * and made with *config, weights of another config, dims l2z_prefill refuses, the sampler's controls as l2z_verify_wide
 * refuses them.  L2Z_ERR_STATE: pos0[j] < 0, pos0[j] + n_tokens[j] > seq_len, a token outside the vocabulary.
 * L2Z_ERR_NO_DEVICE without a device.
 * Out of scope: the product header, map, Zig shim and CLI (ABI version 3); sharded runstates; more than one chunk per call;
 * guesses and verdicts inside a mixed call (l2z_verify_wide); a loop on the device; hipGraph capture; the two attention
 * launches on parallel streams. */
#define L2Z_MIXED_ROWS_MAX 512
int l2z_step_mixed(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                   const float *temperature /* [n] or NULL: all greedy */, const float *top_p /* [n] */,
                   const float *coins /* [n]: one per SEQUENCE */,
                   const l2z_config *config, l2z_runstate *const *states, const l2z_weights *w,
                   int32_t *out_next /* [n] */);

/* ---- paged KV cache: a shared page pool for the wide family (preview) ----
 * A contiguous runstate reserves seq_len rows of K and V in every layer whatever its sequence's length.  A PAGED runstate
 * reserves none: it draws pages of L2Z_KV_PAGE consecutive positions from a pool, on demand, and gives them back.  One page
 * holds, for every layer and kv head, 64 positions of K and the same of V -- [layer][kv head][64][head_size], the
 * contiguous cache's layout with seq_len replaced by 64 --; page p of a sequence covers positions 64 p .. 64 p + 63 (a
 * seq_len that is no multiple of 64 leaves the last page partly used).  The pool's memory is zeroed once at creation;
 * recycled pages are NOT cleared (stale finite rows beyond a sequence's position are covered by the wide family's
 * invariance promises).
 * WHO TAKES THEM.  l2z_prefill_batch, l2z_transformer_wide, l2z_wide_run, l2z_verify_wide and l2z_step_mixed, whose kernels touch a cache
 * in units of 64 absolute positions anyway: a page changes where a block finds its rows and no summation order, so a paged
 * sequence's ids, accepted counts, logits and KV rows are BIT-IDENTICAL to a contiguous one's under the same calls.  All
 * runstates of a call are of one kind -- all contiguous, or all paged from one pool --, else L2Z_ERR_INVALID.  Every other
 * entry point that reads or writes KV rows (l2z_transformer, l2z_prefill, l2z_score, l2z_greedy_begin / _run,
 * l2z_sample_run, l2z_transformer_batch, the l2z_verify family other than l2z_verify_wide, the timing / profile and
 * emulated-rank hooks) refuses a paged runstate with L2Z_ERR_INVALID before it enqueues anything; the logits-only calls
 * (l2z_argmax*, l2z_logits_read / _write, l2z_probs_read, l2z_sample_batch, l2z_synchronize) work unchanged.
 * ATTACHING.  On the host, before anything is enqueued: a call knows every position it writes (pos0[j] .. + rows - 1; every
 * step's for l2z_wide_run), counts the pages still missing, and returns L2Z_ERR_OOM -- nothing enqueued, no page attached,
 * no state changed -- if the pool's free pages fall short; otherwise it attaches them and makes the page tables visible to
 * the device in stream order.  There is no device-side allocation.  After l2z_verify_wide, pages that hold only rejected
 * rows stay attached until a trim.
 * SHARING.  l2z_runstate_fork(dst, src, n_pos) with dst paged: dst first gives back all its pages; with src paged from the
 * same pool the n_pos / 64 whole pages are SHARED (reference counts, no copy) and, if n_pos % 64 != 0, dst gets one private
 * page holding a copy of the rows of the last, partial one; with src contiguous dst attaches ceil(n_pos / 64) pages and the
 * rows are copied in; src paged and dst contiguous: copied out.  Stream ordering and the logits copy are l2z_runstate_fork's
 * own; L2Z_ERR_OOM with nothing changed if pages are short, L2Z_ERR_STATE if a paged src holds no page for a position
 * below n_pos -- as is a call of the wide family whose pos0[j] lies above a page the runstate does not hold (a pass never
 * reads through a missing entry; rows below pos0[j] in pos0[j]'s own page are whatever the page holds).  A call that would WRITE a position inside a page held by more than one runstate is refused with
 * L2Z_ERR_STATE and nothing enqueued (a caller that rewinds below a fork point, a src forked beyond its own position):
 * copy-on-write is out of scope.
 * GIVING BACK.  l2z_runstate_trim, l2z_runstate_free and the dst side of a fork synchronise the runstate's own stream
 * before pages return to the free list -- sufficient, since every pass that read a runstate's pages made that runstate's
 * stream wait for it.  A page is free again when its last holder lets go.
 * l2z_runstate_read("key_cache" / "value_cache") on a paged runstate returns the logical [layer][seq_len][kv_dim] view;
 * unattached positions read as 0.
 * Out of scope: the product header, map, Zig shim and CLI; paged runstates in the single-sequence, batched-16, verify /
 * tree and score paths; sharded runstates; copy-on-write; device-side allocation; eviction or swapping; a scheduler; page
 * sizes other than 64. */
#define L2Z_KV_PAGE 64                      /* positions per page; == the segment of the verify / wide attention */
typedef struct l2z_kvpool l2z_kvpool;
/* n_pages pages for runstates of *config on the current device.  L2Z_ERR_OOM where the device cannot hold them */
int l2z_kvpool_init(const l2z_config *config, int n_pages, l2z_kvpool **out);
/* L2Z_ERR_STATE while a runstate made from it is alive (NULL: nothing to do) */
int l2z_kvpool_free(l2z_kvpool *p);
/* any of the three may be NULL; page_bytes: K and V of one page */
int l2z_kvpool_info(const l2z_kvpool *p, int *n_pages, int *n_free, uint64_t *page_bytes);
/* l2z_runstate_init without key / value caches; L2Z_ERR_INVALID if the pool was made with another config.  Freed by
 * l2z_runstate_free, which gives its pages back */
int l2z_runstate_init_paged(const l2z_config *config, l2z_kvpool *pool, l2z_runstate **out);
/* the page table: page_ids[p] for p < cap = the pool's page that holds positions 64 p .., -1: none */
int l2z_runstate_pages(const l2z_runstate *s, int *n_attached, int32_t *page_ids /* [cap], -1: none */, int cap);
/* give back every page that lies wholly at or above n_pos */
int l2z_runstate_trim(l2z_runstate *s, int n_pos);

/* ---- decode from int8 group-quantized weights: llama2.c version-2 checkpoints (PREVIEW) ----
 * The reference has no quantized path, so nothing here is part of the drop-in boundary: ABI version 2, its 31 functions,
 * the version script, the Zig shim and the CLI are unchanged.
 * GROUP QUANTIZATION of a vector v, per group of `group_size` (32 or 64) consecutive elements: m = max |v_i|,
 * s = m / 127.0f (one correctly rounded f32 division), q_i = round(v_i / s) as int8 (the quotient one correctly rounded f32
 * division, never a multiplication by a reciprocal).  A group with m == 0 -- or with an m so small that s rounds to 0 --
 * has all q_i = 0.  WEIGHTS round half to even (export.py's torch.round), ACTIVATIONS at run time half away from zero
 * (runq.c's round: roundf of the f32 quotient).  Non-finite inputs are UNSPECIFIED.
 * PRODUCT of d rows by n columns: out[i] = sum over groups g of f32(I[i][g]) * ws[i * n / gs + g] * xs[g], with
 * I[i][g] the exact int32 sum over the group of wq * xq; the f32 sum over groups runs in a fixed order that depends on
 * n and gs only (the same bits from run to run).
 * THE PASS is l2z_transformer's with five differences: the embedding row is f32(q) * s of the quantized table's row; the
 * rmsnorm output that feeds q | k | v is quantized over dim and the three products are quantized; the attention output is
 * quantized over dim before Wo; the ffn rmsnorm output over dim before W1 and W3 and the SwiGLU output over hidden_dim
 * before W2; the final rmsnorm output over dim before the classifier, which is the quantized embedding table where the
 * file shares them.  Everything else -- rmsnorm, RoPE, the head-major KV cache, attention, SwiGLU, the residual adds, the
 * argmax rule -- is the f32 pass's.
 * WHO TAKES SUCH WEIGHTS: l2z_transformer, l2z_greedy_begin / _run, l2z_sample_run (prompt positions always step, as under
 * L2Z_PREFILL=0), l2z_time_kind, l2z_profile_forward, with an unsharded, contiguous runstate; the logits-only calls work
 * unchanged; their batched prompt pass is an entry point of its own, l2z_prefill_q8, and so are their batched step and verify
 * pass, l2z_transformer_batch_q8 and l2z_verify_q8 (both below).  Every other entry point that takes weights -- l2z_prefill, l2z_score, l2z_transformer_batch, the verify
 * family, l2z_prefill_batch, the wide family, l2z_step_mixed, the emulated-rank hooks, l2z_weights_read -- refuses them with
 * L2Z_ERR_INVALID before anything is enqueued or changed.  Such weights are unsharded, hold no f32 matrix and no packed
 * copy.
 *
 * l2z_weights_init_q8: `body` is a version-2 file from byte 256 on (the header -- magic 0x616b3432, version 2, the seven
 * config ints, u8 shared_classifier at 36, i32 group_size at 37 -- is the caller's to parse): f32 rms_att_weight [L, dim],
 * rms_ffn_weight [L, dim], rms_final_weight [dim], then each quantized tensor as its int8 values followed by its f32
 * scales: the token embedding, wq, wk, wv, wo, w1, w2, w3 (each layer by layer), wcls unless shared.  L2Z_ERR_INVALID for
 * a group size other than 32 / 64, dim or hidden_dim no multiple of it, a body shorter than the config needs, a non-null
 * comm.
 * l2z_weights_init_q8_from: quantizes an unsharded f32 weights object ON THE DEVICE (the weight rule); the result is
 * independent of the source.
 * l2z_weights_q8_read: tensor `tensor_name` ("token_embedding_table", "wq", "wk", "wv", "wo", "w1", "w2", "w3", "wcls") of
 * `layer` in the FILE's row order: rows * cols int8 into out_q, rows * cols / group_size scales into out_s.
 * l2z_q8_quantize: the activation rule on its own (n a multiple of gs).  l2z_q8_matmul: the product on its own, through
 * the kernel body the pass launches (host pointers; xq [n], xs [n / gs], wq [d * n], ws [d * n / gs]). */
int l2z_weights_init_q8(const l2z_config *config, const void *body, size_t n_bytes, int shared_classifier, int group_size,
                        const l2z_comm *comm, l2z_weights **out);
int l2z_weights_init_q8_from(const l2z_weights *w_f32, int group_size, l2z_weights **out);
int l2z_weights_q8_read(const l2z_weights *w, const char *tensor_name, int layer, int8_t *out_q, float *out_s);
int l2z_q8_quantize(const float *x, size_t n, int gs, int8_t *out_q, float *out_s);
int l2z_q8_matmul(float *out, const int8_t *xq, const float *xs, const int8_t *wq, const float *ws, size_t n, size_t d, int gs);

/* l2z_q8_matvec_case: ONE launch of the quantized mat-vec as the pass issues it, every argument the caller's; host
 * pointers, synchronous.  epi: 0 store, 1 RoPE + KV write, 2 residual, 3 SwiGLU, 4 classifier with argmax candidates.
 * Segments: q0 / s0 [rows0][n] and [rows0][n / gs], likewise q1, q2 (rows1, rows2; 0: unused).  SwiGLU: rows0 == rows1
 * pairs, q0 / s0 the ONE slot of 2 * rows0 rows with W1 and W3 row-interleaved, out0 [rows0].  Residual and argmax take
 * one segment.  x in one of three forms: quantized already (xq [n], xs [n / gs]; x and rms_w null), f32 (x [n]), or f32
 * with the rmsnorm in the kernel (x and rms_w [n]).
 * out0 / out1 / out2 hold out0_len / out1_len / out2_len floats and are IN and OUT: they are uploaded as they stand, the
 * launch writes its rows, and everything comes back, so what the launch must not touch can be checked.  RoPE: `rope` is
 * (pos + 1) * head_size / 2 {cos, sin} pairs, the leading rope_segs segments are rotated, out0 is q [rows0], out1 / out2
 * are one layer's head-major caches [rows / head_size][seq_len][head_size] (kv_head_stride = seq_len * head_size,
 * pos_stride = head_size, as the pass sets them); every segment holds whole heads.  Residual: out0 = resid + W.x, resid
 * [rows0]; in_place != 0: resid is not read, out0 is both (out0 == resid on the device, as the pass's Wo and W2 launches).
 * Argmax: out0 the logits, part_val / part_idx (room for part_cap) get the `grid` per-block candidates.
 * max_blocks_per_cu, n_cus: what the launcher sizes its grid from; 0: the pass's own (8, the device's CU count).
 * grid (out): the blocks launched. */
typedef struct {
    int epi, gs, n, rows0, rows1, rows2;
    const int8_t *q0, *q1, *q2;
    const float *s0, *s1, *s2;
    const int8_t *xq;
    const float *xs, *x, *rms_w;
    int pos, head_size, rope_segs, seq_len;
    const float *rope;
    const float *resid;
    int in_place;
    int max_blocks_per_cu, n_cus;
    float *out0, *out1, *out2;
    size_t out0_len, out1_len, out2_len;
    float *part_val;
    int *part_idx;
    int part_cap;
    int grid;
} l2z_q8_case;
int l2z_q8_matvec_case(l2z_q8_case *c);

/* ---- Batched prompt pass on int8 group-quantized weights (PREVIEW) ----
 * l2z_prefill_q8: the state change of l2z_transformer(tokens[i], pos0 + i, ...) on q8 weights for i = 0 .. n_tokens - 1
 * -- KV rows pos0 .. pos0 + n_tokens - 1 of every layer written, the LAST position's logits (and the classifier's argmax
 * candidates) in the runstate, so l2z_argmax, l2z_logits_read, l2z_probs_read and l2z_sample_batch work on them and
 * l2z_transformer or l2z_sample_run may go on from pos0 + n_tokens -- with every weight matrix streamed once per chunk
 * (l2z_prefill's chunk plan, at most 1024 rows) and multiplied on the int8 matrix cores.
 * THE ARITHMETIC is the definition above, row by row: each row's activations are quantized by the activation rule over
 * dim before q | k | v, Wo, W1 | W3 and the classifier and over hidden_dim before W2, and a product is
 * sum_g f32(I_g) * ws * xs with exact integer group sums.  The f32 sum over groups runs in another (fixed) order than the
 * stepped pass's, so the two agree up to f32 summation order, not bit for bit; the same bits from run to run.
 * l2z_prefill, l2z_greedy_run and every other entry point are unchanged: they refuse such weights or step the prompt.
 * A refusal enqueues nothing and changes nothing.  L2Z_ERR_NO_DEVICE without a device; L2Z_ERR_INVALID for a null
 * argument, n_tokens < 1, f32 or packed weights (those go to l2z_prefill), a sharded or paged runstate, a config other
 * than the objects'; L2Z_ERR_STATE for positions outside [0, seq_len) or a token outside the vocabulary.
 *
 * l2z_q8_quantize_rows: the pass's row launch on its own (host pointers): m rows of n floats -> out_q [m, n] and out_s
 * [m, n / gs] by the activation rule, after the rmsnorm with rms_w [n] where that is not null.
 * l2z_q8_gemm: the pass's GEMM on its own, store epilogue (host pointers): out [m, d] from m quantized rows (xq [m, n],
 * xs [m, n / gs]) and d quantized weight rows (wq [d, n], ws [d, n / gs]); d a multiple of 4.  The order of a row's f32
 * sum depends on n and gs only: a row's bits do not depend on m or on the other rows. */
int l2z_prefill_q8(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
                   const l2z_weights *w);
int l2z_q8_quantize_rows(const float *x, int m, size_t n, const float *rms_w, int gs, int8_t *out_q, float *out_s);
int l2z_q8_gemm(float *out, const int8_t *xq, const float *xs, int m, const int8_t *wq, const float *ws, size_t n, size_t d,
                int gs);

/* ---- Batched and speculative decoding on int8 group-quantized weights (PREVIEW) ----
 * The batched step of l2z_transformer_batch on q8 weights, under names of its own: l2z_transformer_batch, the l2z_verify
 * family and every other entry point keep refusing such weights.
 * l2z_transformer_batch_q8: l2z_transformer_batch's contract -- 1 .. L2Z_BATCH_MAX sequences, one runstate each, one token
 * each at its own position; each row's KV rows in its own caches and its WHOLE logits in its own runstate, so
 * l2z_argmax_batch, l2z_sample_batch, l2z_argmax and l2z_logits_read work behind it.
 * l2z_verify_q8: l2z_verify's contract -- 1 .. L2Z_BATCH_MAX consecutive positions of ONE sequence in one sweep of the
 * weights, the verdict on the device -- with temperature 0 and coins NULL, l2z_verify_sample's with a temperature (coins[i]:
 * the coin of position pos0 + i).  l2z_verify_logits_read serves its rows.
 * THE ARITHMETIC is 4.23's definition row by row, as l2z_prefill_q8's: rows quantized by the activation rule, a product
 * sum_g f32(I_g) * ws * xs with exact integer group sums and the f32 sum in l2z_q8_gemm's order -- the bits of a row's
 * product are those l2z_q8_gemm gives for the same quantized row and matrix --, f32 attention (l2z_transformer_batch's
 * and l2z_verify's kernels).  A row's results do not depend on the other rows of the call, on their number or on its
 * place among them.
 * A refusal enqueues nothing and changes nothing.  L2Z_ERR_NO_DEVICE without a device; L2Z_ERR_INVALID for a null argument,
 * n / n_tokens outside [1, L2Z_BATCH_MAX], f32 or packed weights (those go to l2z_transformer_batch / l2z_verify), a sharded
 * or paged runstate, a config other than the objects', a head_size that is no multiple of 4 or above 256, a vocab_size
 * that is no multiple of 4, l2z_sample_batch's rules for temperature, top_p and the coins; L2Z_ERR_STATE for a position
 * outside [0, seq_len) or a token outside the vocabulary.
 * l2z_batch_q8_time / l2z_verify_q8_time (scripts/q8_batch_bench.py): the twins of l2z_batch_time / l2z_verify_time --
 * one call, then `iters` passes back to back, timed by device events on the pass's stream. */
int l2z_transformer_batch_q8(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                             l2z_runstate *const *states, const l2z_weights *w);
int l2z_verify_q8(const int32_t *tokens, int n_tokens, int pos0, float temperature, float top_p, const float *coins,
                  const l2z_config *config, l2z_runstate *s, const l2z_weights *w, int32_t *out_next, int *out_accepted);
int l2z_batch_q8_time(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config, l2z_runstate *const *states,
                      const l2z_weights *w, int iters, double *out_ms);
int l2z_verify_q8_time(const int32_t *tokens, int n_tokens, int pos0, float temperature, float top_p, const float *coins,
                       const l2z_config *config, l2z_runstate *s, const l2z_weights *w, int iters, double *out_ms);

#ifdef __cplusplus
}
#endif
#endif /* LLAMA2_HIP_TEST_H */
