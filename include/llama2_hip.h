/*
 * llama2_hip.h -- C ABI of the MI355X (gfx950) forward pass for cgbur/llama2.zig.
 *
 * The reference has no FFI today: the boundary is the Zig-internal call
 *     transformer(token, pos, *Config, *RunState, *Weights) void     src/main.zig:285
 * with its sole call site at src/main.zig:996.  This header gives that call,
 * and the three objects it takes, a C ABI with the same names, argument
 * meaning and ownership, so a maintainer replaces each Zig call by the
 * matching extern (INTEGRATION.md shows the Zig `extern fn` block).
 *
 *   reference (src/main.zig)                 this library
 *   ---------------------------------------  -----------------------------------
 *   ConfigReader / Config        :17-49      l2z_config (same 7 x i32 layout)
 *   Weights.init(config,data,shared) :73     l2z_weights_init      (uploads to HBM)
 *   RunState.init(alloc,config)  :137        l2z_runstate_init     (device buffers)
 *   RunState.deinit              :156        l2z_runstate_free
 *   transformer(token,pos,c,s,w) :285        l2z_transformer
 *   argmax(state.logits)         :715,:1003  l2z_argmax            (on device)
 *   state.logits after return    :1005-1012  l2z_logits_read       (D2H, for samplers)
 *   logits / temperature, softmax :1005-1008  l2z_probs_read        (on the device, then D2H)
 *   while (pos < seq_len) loop at -t 0 :995  l2z_greedy_begin / l2z_greedy_run
 *   (no reference equivalent)                l2z_score             (log-prob and top-1 of every position of a text)
 *   (no reference equivalent)                l2z_verify            (several positions of one sequence per sweep: speculation)
 *   (no reference equivalent)                l2z_verify_sample     (the same under the sampler: -t / -p speculation)
 *   matmul, rmsnorm, softmax, ... :432-726   kernel-level hooks of the same names, for tests only:
 *                                            include/llama2_hip_test.h
 *
 * Ownership: the caller owns config; weights and runstate handles own their
 * device memory.  The host blob passed to l2z_weights_init may be freed (or
 * un-mmapped) as soon as the call returns.  One runstate = one sequence, used
 * from one thread at a time, pos strictly increasing from 0 -- exactly the
 * reference's contract (main.zig:994-995).
 *
 * Errors: the reference's transformer() cannot fail; a device path can.  Every
 * entry point returns L2Z_OK (0) or a negative l2z_status; l2z_last_error()
 * returns a thread-local message.  There is NO CPU fallback: without a gfx950
 * device every compute entry point fails with L2Z_ERR_NO_DEVICE.
 *
 * All floats are IEEE f32, exactly as in the checkpoint.
 */
#ifndef LLAMA2_HIP_H
#define LLAMA2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L2Z_ABI_VERSION 2

typedef enum l2z_status {
    L2Z_OK = 0,
    L2Z_ERR_INVALID = -1,    /* bad argument / shape the kernels do not support */
    L2Z_ERR_NO_DEVICE = -2,  /* no HIP device, or device is not usable */
    L2Z_ERR_HIP = -3,        /* a HIP runtime call failed */
    L2Z_ERR_OOM = -4,        /* device or host allocation failed */
    L2Z_ERR_COMM = -5,       /* RCCL failure (multi-GPU only) */
    L2Z_ERR_STATE = -6       /* call sequence violates the contract (e.g. pos out of range) */
} l2z_status;

/* src/main.zig:17-25 ConfigReader: 7 x i32, little endian, the first 28 bytes
 * of a checkpoint.  vocab_size here is already abs()'d (main.zig:944); the
 * sign is passed separately as `shared_weights` (main.zig:943). */
typedef struct l2z_config {
    int32_t dim;        /* transformer dimension */
    int32_t hidden_dim; /* ffn hidden dimension */
    int32_t n_layers;
    int32_t n_heads;
    int32_t n_kv_heads; /* <= n_heads, divides it (GQA) */
    int32_t vocab_size;
    int32_t seq_len;    /* max sequence length = KV-cache rows per layer */
} l2z_config;

typedef struct l2z_weights l2z_weights;   /* src/main.zig:53  Weights, resident in HBM */
typedef struct l2z_runstate l2z_runstate; /* src/main.zig:119 RunState, resident in HBM */
typedef struct l2z_comm l2z_comm;         /* multi-GPU shard group (no reference equivalent) */

/* ---- library / device ---- */
int l2z_abi_version(void);
const char *l2z_last_error(void);
int l2z_device_count(int *out_n);
/* name (<= cap bytes), CU count, HBM bytes of device `dev` */
int l2z_device_info(int dev, char *name, size_t cap, int *out_cus, uint64_t *out_hbm_bytes);

/* ---- Weights: src/main.zig:73 Weights.init(config, data, shared_weights) ----
 * `data` is the f32 blob that follows the 28-byte header, n_floats long, in
 * the Weights.init carve order (main.zig:85-112) including the unused
 * freq_cis region.  comm == NULL: the whole blob is uploaded as ONE device
 * allocation with the same layout.  comm != NULL: only this rank's rows of
 * every matrix are uploaded (heads / output rows, DESIGN.md "Sharding"). */
int l2z_weights_init(const l2z_config *config, const float *data, size_t n_floats,
                     int shared_weights, const l2z_comm *comm, l2z_weights **out);
void l2z_weights_free(l2z_weights *w);

/* ---- RunState: src/main.zig:137 RunState.init / :156 deinit ----
 * Allocates x, xb, hb, q, att, logits and the (layer, seq_len, kv_dim) key and
 * value caches in HBM, plus the RoPE cos/sin table (seq_len, head_size/2) that
 * replaces the per-layer pow/cos/sin of main.zig:338-342. */
int l2z_runstate_init(const l2z_config *config, const l2z_comm *comm, l2z_runstate **out);
void l2z_runstate_free(l2z_runstate *s);

/* ---- src/main.zig:285 transformer(token, pos, config, s, w) ----
 * One decoder forward pass; on return the logits for `pos` are in the
 * runstate (device) and the KV-cache rows `pos` are written in every layer.
 * Asynchronous on the runstate's stream; l2z_argmax / l2z_logits_read sync. */
int l2z_transformer(int token, int pos, const l2z_config *config, l2z_runstate *s,
                    const l2z_weights *w);
/* src/main.zig:715 argmax over s.logits, on device.  THE RULE, for every call of this header that returns a token id from
 * a row of logits at temperature 0 (l2z_argmax, l2z_greedy_run, l2z_argmax_batch, l2z_sample_batch, l2z_verify*) and for
 * l2z_score's top-1: what the reference's scan (max = x[0], then strict '>') returns on the row's f32 values --
 *   index 0 if x[0] is a NaN; otherwise the lowest index of the largest non-NaN value (a NaN behind index 0 never wins,
 *   the first of equal maxima does; +-inf, signed zeros and denormals compare as IEEE values); index 0 if the row holds
 *   no non-NaN value.
 * At a temperature the id is the host sampler's on l2z_probs_read's probabilities with no tolerance, all-NaN
 * probabilities included (a NaN or +inf among the logits, or nothing but -inf): sample returns vocab_size - 1,
 * sample_top_p the argmax of the probabilities, 0.
 * SHARDED runstates: l2z_argmax, l2z_logits_read and l2z_probs_read are COLLECTIVE after greedy steps
 * (l2z_greedy_run) on the peer-write transport -- those steps exchange one argmax candidate per rank instead of
 * gathering the logits, so the first call that needs the whole vector gathers it, and every rank of the group
 * must make that call (as every rank makes every other call); a rank that calls alone waits L2Z_P2P_TIMEOUT_S
 * and gets L2Z_ERR_COMM.  After l2z_transformer / l2z_prefill the logits are already whole: plain reads. */
int l2z_argmax(l2z_runstate *s, int *out_token);
/* copy s.logits (vocab_size floats) to the host (sharded: see l2z_argmax) */
int l2z_logits_read(l2z_runstate *s, float *out_logits);
/* src/main.zig:1005-1008 on the device: out_probs[i] = softmax(logits / temperature)[i] (temperature > 0),
 * then the device-to-host copy of vocab_size floats; the caller goes on with sample / sample_top_p
 * (:1009-1012).  32000 exp() on one host core take longer than a small model's forward pass. */
int l2z_probs_read(l2z_runstate *s, float temperature, float *out_probs);
/* ---- src/main.zig:987-1042, the generation loop at temperature 0 ----
 * Runs entirely on the device: the forward pass, argmax, the prompt override
 * (main.zig:999-1000) and the token/pos hand-over to the next step are one
 * hipGraph replayed per position, with no host round trip per token.
 *   l2z_greedy_begin : token = BOS(1), pos = 0, install the prompt
 *   l2z_greedy_run   : run `n_steps` more positions, write `next` of each to
 *                      out_tokens; stops early after a BOS (main.zig:1017) and
 *                      at seq_len; *out_n = positions actually produced.
 */
int l2z_greedy_begin(l2z_runstate *s, const int32_t *prompt, int n_prompt);
int l2z_greedy_run(const l2z_config *config, l2z_runstate *s, const l2z_weights *w, int n_steps,
                   int32_t *out_tokens, int *out_n);

/* ---- batched prefill (no reference equivalent: src/main.zig:999-1000
 * feeds the prompt one token at a time) ----
 * Same state change as l2z_transformer(tokens[i], pos0 + i) for i = 0 .. n_tokens-1 -- the
 * KV-cache rows pos0 .. pos0+n_tokens-1 of every layer are written and the logits of the LAST
 * position are left in the runstate (l2z_argmax / l2z_logits_read) -- but each weight matrix is
 * streamed once per chunk of up to 1024 tokens and multiplied as a dense GEMM on the matrix cores:
 * the fp32 ones (v_mfma_f32_32x32x2_f32) for models whose matrices stay in the caches; for matrices
 * that stream from HBM the bf16 ones, f32-ACCURATELY -- both operands cut into three bf16 terms
 * (exact splits), the six products of order >= 2^-16 summed in f32 (error against float64 not above
 * the fp32 cores' own chain; L2Z_PF_X3=0 in the environment keeps the fp32 cores everywhere).  Values
 * agree with the token-by-token path up to summation order.  Dims must be multiples of 4 (else L2Z_ERR_INVALID, and the caller loops over
 * l2z_transformer).  On a sharded runstate every rank of the group makes the same call: the pass is
 * row-sharded like the decode pass and bit-identical to the unsharded one; it needs a transport for
 * [1024, hidden_dim] matrices -- the peer-write arena's bulk regions (allocated by
 * l2z_comm_p2p_export unless L2Z_P2P_BULK_MB=0) or an RCCL communicator -- else L2Z_ERR_INVALID.
 * l2z_greedy_run uses the same pass for the prompt positions when its first call after
 * l2z_greedy_begin asks for at least n_prompt steps, n_prompt >= L2Z_PREFILL_MIN_PROMPT and no
 * prompt token is BOS; L2Z_PREFILL=0 in the environment keeps the stepped loop. */
#define L2Z_PREFILL_MIN_PROMPT 4
int l2z_prefill(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config,
                l2z_runstate *s, const l2z_weights *w);

/* ---- scoring a token sequence (no reference equivalent: the reference only generates) ----
 * STATE CHANGE: exactly l2z_prefill(tokens, n_tokens, pos0, ...) -- the KV-cache rows pos0 .. pos0+n_tokens-1 of every
 * layer and the runstate's logits (last position) are bit-identical to what l2z_prefill leaves (same chunks, same
 * launches per layer), so a caller scores a prompt and goes on generating from it, forks it or batches it.
 * OUTPUTS, for i = 0 .. n_tokens-1, with z_i the f32 logits of position pos0+i (final rmsnorm of the residual row, times
 * the classifier matrix -- the embedding when the checkpoint shares them -- by the prefill pass's GEMM kernels):
 *   out_logprob[i] = z_i[targets[i]] - (m_i + log sum_v exp(z_i[v] - m_i)),  m_i = max_v z_i[v], all in f32; the sums
 *                    run in a fixed order that depends on vocab_size only (same bits run to run, whatever the workspace).
 *                    targets[i] == -1: no target at this position, out_logprob[i] = 0.  The usual call passes
 *                    targets[i] = tokens[i+1] and -1 for the last.
 *   out_top1[i]    = argmax_v z_i[v], strict '>', lowest index wins (l2z_argmax's rule).
 * out_logprob may be NULL iff targets is NULL; out_top1 may be NULL; not both absent.  Synchronous (the outputs are host
 * arrays).  The logits never exist as a [n_tokens, vocab] matrix: the classifier product is written one slab of
 * vocabulary rows at a time into a workspace of at most 64 MB (32 MB + the per-row partials at the default chunking),
 * allocated on the runstate's first l2z_score call and freed with it.
 * Contract (a refusal enqueues nothing and changes no state): L2Z_ERR_INVALID for NULL tokens, n_tokens < 1, both outputs
 * absent, targets without out_logprob or the reverse, a sharded runstate (comm != NULL), dims l2z_prefill refuses;
 * L2Z_ERR_STATE for positions outside [0, seq_len), a token outside the vocabulary, a target outside {-1} u [0, vocab_size).
 * OUT OF SCOPE: sharded runstates (the vocabulary rows are sharded there: it would take an exchange of one (max, sum,
 * argmax, target logit) tuple per rank and row), and a batch of sequences per call -- callers loop; N continuations of one
 * prompt: score the prompt once, l2z_runstate_fork, score each continuation with pos0 = n_prompt. */
int l2z_score(const int32_t *tokens, int n_tokens, int pos0, const int32_t *targets,
              const l2z_config *config, l2z_runstate *s, const l2z_weights *w,
              float *out_logprob, int32_t *out_top1);

/* wait for everything queued on the runstate's stream */
int l2z_synchronize(l2z_runstate *s);

/* ---- batched decode (no reference equivalent: the reference steps one sequence) ----
 * Up to L2Z_BATCH_MAX independent sequences, one runstate each, advanced by one token with ONE sweep of the weights.
 * Same state change as l2z_transformer(tokens[i], pos[i], config, states[i], w) for i = 0 .. n-1: KV row pos[i] of
 * every layer is written in states[i] and no other cache row is touched; states[i]'s logits hold its result, and
 * l2z_argmax / l2z_logits_read / l2z_probs_read work on it unchanged.  A runstate moves freely between l2z_prefill,
 * l2z_transformer and batched steps.
 * Contract (else L2Z_ERR_INVALID, or L2Z_ERR_STATE for pos / tokens, with no state changed and nothing enqueued):
 * 1 <= n <= L2Z_BATCH_MAX; the runstates pairwise distinct, unsharded (comm == NULL), on one device and made with
 * *config; 0 <= pos[i] < seq_len and 0 <= tokens[i] < vocab_size; dims l2z_prefill accepts (multiples of 4,
 * head_size <= 256).
 * Streams: the pass waits for everything queued on every runstate's stream, and every runstate's stream waits for the
 * pass (events, no device-wide sync), so later calls on any of them see its results.
 * BATCH INVARIANCE: a sequence's logits and KV rows are bit-identical whether it runs alone (n = 1) or in a batch of
 * 2 ... 16, whatever the other sequences hold, and in any order within the batch (every product takes one kernel form
 * and one summation order independent of n).  They equal l2z_transformer's up to summation order (the fp32 parity
 * bar), not bit for bit. */
#define L2Z_BATCH_MAX 16
int l2z_transformer_batch(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                          l2z_runstate *const *states, const l2z_weights *w);
/* out_tokens[i] = argmax of states[i]'s logits (strict '>', lowest index wins): one launch, one sync.  The runstates
 * follow l2z_transformer_batch's rules (distinct, unsharded, one device, one config). */
int l2z_argmax_batch(int n, l2z_runstate *const *states, int32_t *out_tokens);
/* src/main.zig:1002-1012 on the device for n runstates, one launch, one sync: out_tokens[i] = the token the host
 * samplers draw from states[i]'s logits with temperature[i], top_p[i] and the random number coins[i] (the
 * std.Random.float(f32) value the reference draws, :731 / :789):
 *   temperature[i] == 0: the argmax, as l2z_argmax_batch (the coin is not used);
 *   else probs = softmax(logits / temperature[i]), bit for bit what l2z_probs_read returns, then
 *   top_p[i] == 0 or 1: sample (:728-741): the first token whose cdf (a sequential f32 sum in token order) exceeds
 *                       the coin, else vocab_size - 1;
 *   otherwise:          sample_top_p (:754-798) with the candidates ordered by (probability descending, token id
 *                       ascending), the host sampler's total order, and its sequential f32 sums.
 * The logits are not modified.  A row's token depends on its own runstate and arguments alone (BATCH INVARIANCE).
 * Contract (else L2Z_ERR_INVALID with nothing enqueued): the runstates follow l2z_transformer_batch's rules;
 * temperature[i] finite and >= 0, top_p[i] in [0, 1], coins[i] in [0, 1).  Streams as in l2z_transformer_batch. */
int l2z_sample_batch(int n, l2z_runstate *const *states, const float *temperature, const float *top_p,
                     const float *coins, int32_t *out_tokens);
/* dst becomes a copy of src's first n_pos positions: KV-cache rows 0 .. n_pos-1 of every layer and src's logits
 * (device to device, no sync).  dst's rows >= n_pos are not touched; its next position is n_pos, so it continues
 * src's sequence from there (N samples of one prompt run the prompt once).  The greedy loop's state is not copied
 * (l2z_greedy_begin starts it over).  dst's stream waits for src's, and src's for the copies.
 * Contract: dst and src distinct, unsharded, on one device, made with one config (else L2Z_ERR_INVALID);
 * 0 <= n_pos <= seq_len (else L2Z_ERR_STATE); nothing is enqueued on a refusal. */
int l2z_runstate_fork(l2z_runstate *dst, const l2z_runstate *src, int n_pos);

/* ---- speculative greedy decoding: verify up to L2Z_BATCH_MAX - 1 guessed tokens of ONE sequence in one sweep ----
 * One sequence, n_tokens consecutive positions, one sweep of the weights.
 * tokens[0] is the sequence's token at pos0 (known); tokens[1 .. n_tokens-1] are GUESSES for pos0+1 ...
 * Row i computes z_i = the logits of position pos0+i given tokens[0..i] on top of the cache rows < pos0,
 * next_i = argmax z_i (strict '>', lowest index: l2z_argmax's rule).
 * *out_accepted = a = the largest a in [0, n_tokens-1] with tokens[j] == next_{j-1} for all 1 <= j <= a.
 * out_next[0 .. n_tokens-1] = next_i; entries 0 .. a are the sequence's next a+1 tokens, the rest are what the model
 * would have said after a wrong guess (diagnostic only).
 * STATE on return: KV rows pos0 .. pos0+a of every layer are the sequence's; the runstate's logits are z_a
 * (l2z_argmax == out_next[a]; l2z_logits_read / l2z_probs_read / l2z_sample_batch work on them); the next position is
 * pos0+a+1.  Rows pos0+a+1 .. pos0+n_tokens-1 have been written with the rejected guesses' keys and values: they are
 * beyond the next position, which every entry point overwrites before it reads (pos strictly increasing).  No row
 * < pos0 and no row >= pos0+n_tokens is touched.  Synchronous (one copy back, one sync).
 * The products are the batched step's (one kernel form whatever n_tokens is); attention is a multi-query, causal form
 * split over fixed segments of absolute positions that reads each K / V row once per call (flash arithmetic: agrees
 * with l2z_transformer up to summation order, the fp32 parity bar, not bit for bit).
 * DRAFT INVARIANCE: z_i and the K / V rows of position p = pos0+i are a function of the model, the tokens at positions
 * 0 .. p and p alone.  They do not depend on n_tokens, on i, on pos0, on the guesses behind row i, or on how earlier
 * positions were cut into calls -- provided the earlier positions were themselves produced by l2z_verify (rows produced
 * by l2z_prefill / l2z_transformer are inputs like any other: same inputs, same bits).  Consequence: a greedy loop over
 * l2z_verify emits the same ids, and ends with the same logits and cache bits, for every drafter and every number of
 * guesses, none included.  Speculation changes the time, never the text.
 * Contract (a refusal enqueues nothing and changes no state): L2Z_ERR_INVALID for NULL arguments, n_tokens outside
 * [1, L2Z_BATCH_MAX], a sharded runstate, dims l2z_transformer_batch refuses; L2Z_ERR_STATE for pos0 < 0,
 * pos0 + n_tokens > seq_len, a token outside the vocabulary; L2Z_ERR_NO_DEVICE without a device.
 * Scratch (on the runstate's first call, freed with it): the batched step's activation rows, L2Z_BATCH_MAX x vocab_size
 * floats of logits, the attention partials.
 * OUT OF SCOPE: several sequences per call (the preview entry point l2z_verify_batch of llama2_hip_test.h does that, with
 * this call's bits per sequence), sharded runstates, hipGraph replay of the pass (its grid depends on pos0). */
int l2z_verify(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
               const l2z_weights *w, int32_t *out_next, int *out_accepted);
/* ---- speculative decoding under the sampler: l2z_verify with every row DRAWN instead of arg-maxed ----
 * The pass, the KV rows written, out_accepted's definition, the STATE on return (logits = z_a, next position pos0+a+1),
 * synchronisation and scratch are l2z_verify's.  The one difference: next_i = the token l2z_sample_batch draws from z_i
 * with (temperature, top_p, coins[i]) -- that launch's kernel, on the n rows of the pass, so the host sampler's bits.
 * THE RULE.  A drafter that proposes ONE token x per position as a function of the earlier tokens only (prompt lookup,
 *   any deterministic callable, a draft model decoded greedily) has the draft distribution q = delta_x.  Rejection
 *   sampling then accepts x with probability min(1, p(x) / q(x)) = p(x), else draws from max(0, p - q) renormalised = p
 *   restricted to tokens != x.  That is the law of: draw y from p with the position's own random number; y == x accepts
 *   the guess, otherwise y is the token.  No ratio, no residual distribution; p is what the sampler samples from.
 * Give every POSITION its own coin -- coin g belongs to the g-th generated token, as the plain loop draws one per token
 * (main.zig:731 / :789) -- and pass row i the coin of position pos0+i.  A row behind a rejected guess is discarded and its
 * position drawn again by the next call WITH THE SAME COIN.  Then the law of the text is the plain sampler's, provided the
 * drafter never looks at the coins, and
 * COIN INVARIANCE: given the model, the prompt, temperature, top_p and the coin sequence, the ids do not depend on the
 * number of guesses or on the drafter, nor do the final logits and the cache rows below the next position, bit for bit
 * (z_i depends on the tokens at 0 .. pos0+i alone: DRAFT INVARIANCE; the draw on z_i and its position's coin alone:
 * l2z_sample_batch's BATCH INVARIANCE).  Speculation changes the time, never the text.
 * Against the reference's stream of numbers the position-indexed coins differ in one place: sample_top_p with no
 * candidate above its cutoff (the reference asserts there, :771) returns the argmax and draws nothing.  That takes top_p < 1 / vocab_size (the
 * largest probability is at least 1 / vocab_size, up to rounding); here the position's coin is simply not used.
 * temperature == 0: next_i is the argmax and coins may be NULL; outputs, logits and cache bits equal l2z_verify's on the
 * same arguments (its launches).
 * Contract, on top of l2z_verify's (a refusal enqueues nothing and changes no state): L2Z_ERR_INVALID for a temperature
 * that is not finite or < 0, top_p outside [0, 1], coins == NULL with temperature > 0, a coins[i] outside [0, 1).
 * Scratch: l2z_verify's and l2z_sample_batch's (5 x vocab_size floats per row).
 * OUT OF SCOPE: a drafter that itself samples (the general p / q rule with the draft's probabilities on the device),
 * several sequences per call, sharded runstates, hipGraph replay, log-probs of the emitted tokens. */
int l2z_verify_sample(const int32_t *tokens, int n_tokens, int pos0, float temperature, float top_p,
                      const float *coins, const l2z_config *config, l2z_runstate *s, const l2z_weights *w,
                      int32_t *out_next, int *out_accepted);

/* ---- multi-GPU shard group: one process per GPU, xGMI ----
 * The reference is single-threaded and single-device; this is what the build
 * adds.  Two transports for the per-layer all-gathers:
 *  - RCCL: id is an opaque 128-byte ncclUniqueId made on rank 0 and distributed by the launcher
 *    (bench.py uses torch.distributed/gloo for that);
 *  - peer writes: l2z_comm_init(rank, world, NULL, device, &c), then every rank exports the IPC
 *    handle of its landing arena (l2z_comm_p2p_export), the launcher all-gathers the 64-byte
 *    handles in rank order, and l2z_comm_p2p_connect maps the peers.  A gather is then one small
 *    kernel of direct 8-byte {value, epoch} stores into the peers' memory, polled by the receiver --
 *    no fences, no collective library, and it can be captured in the step graph.  Preferred when both are set up (L2Z_COMM=rccl overrides).
 *    max_vector_floats must be >= max(dim, hidden_dim, vocab_size) of every config used with the
 *    group: l2z_runstate_init refuses (L2Z_ERR_COMM) a config the landing slots cannot hold.
 *    The arena also carries two bulk regions of max_vector_floats x 1024 floats (L2Z_P2P_BULK_MB
 *    overrides, 0 = none) for the sharded prefill's activation matrices: plain 16-byte peer stores
 *    and one flag per sender.
 */
#define L2Z_COMM_ID_BYTES 128
int l2z_comm_unique_id(void *out_id);
int l2z_comm_init(int rank, int world, const void *id, int device, l2z_comm **out);
#define L2Z_COMM_IPC_BYTES 64
/* max_vector_floats: the longest vector that will be gathered = max(dim, hidden_dim, vocab_size) */
int l2z_comm_p2p_export(l2z_comm *c, size_t max_vector_floats, void *handle_out);
/* the same with the bulk regions sized separately: max_matrix_width = max(dim, hidden_dim), the widest
 * [tokens, n] matrix the sharded prefill gathers (the vocabulary only ever travels as a vector), so the
 * arena holds 2 x max_matrix_width x 1024 floats of bulk space instead of 2 x max_vector_floats x 1024 */
int l2z_comm_p2p_export_sized(l2z_comm *c, size_t max_vector_floats, size_t max_matrix_width, void *handle_out);
int l2z_comm_p2p_connect(l2z_comm *c, const void *handles /* world x L2Z_COMM_IPC_BYTES */);
int l2z_comm_rank(const l2z_comm *c, int *rank, int *world);
void l2z_comm_free(l2z_comm *c);
/* Pure host logic, no GPU needed: the row range [*r0,*r1) of a `rows`-row
 * tensor owned by `rank` of `world`, in units of `granule` rows (head_size for
 * q/k/v so shards are whole heads, 1 otherwise).  Fails if not divisible. */
int l2z_shard_range(int64_t rows, int64_t granule, int rank, int world, int64_t *r0, int64_t *r1);

#ifdef __cplusplus
}
#endif
#endif /* LLAMA2_HIP_H */
