// verify_host.cpp -- host side of the verify family: the batched step (batch_host.cpp's batch_step) with the rows being
// guessed positions, and the verdict on the device.  l2z_verify / l2z_verify_sample: consecutive positions of ONE sequence
// (verify.hip).  l2z_verify_batch: that for the rows of several sequences at once, attention and verdict per sequence
// (verify_batch.hip).  l2z_verify_tree: the nodes of a tree of guesses on one sequence, with the compaction of the accepted
// path (verify_tree.hip).  Every path reads the same way: checks (a refusal enqueues nothing and changes no state), scratch,
// table, the step with the path's attention, the rows' next ids (verify_ids), the path's accept kernel, the copy back.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "batch_host.h"

namespace l2z {
namespace {

// How a pass finds its rows' next ids: at temperature 0 the argmax (the greedy verdict), else l2z_sample_batch's draw from
// the row's logits with the coin the path gives the row
struct VerifyDraw {
    float temperature, top_p;
    const float *coins;
    bool sampled() const { return temperature > 0.0f; }
};
const VerifyDraw kGreedy = {0.0f, 0.0f, nullptr};

// ---- the preconditions the paths share; fn: the entry point a message names ----

// the runstates of a pass against its config and weights, then what the step asks of the first
int check_targets(const char *fn, const l2z_config *config, int n, l2z_runstate *const *states, const l2z_weights *w)
{
    for (int j = 0; j < n; j++) L2Z_TRY(check_pair(config, states[j], w));
    L2Z_TRY(prefill_check(config, states[0]));
    L2Z_CHECK(states[0]->sh.hs <= 256, L2Z_ERR_INVALID, "%s: head_size above 256", fn);
    return L2Z_OK;
}

// ... for a pass on one runstate; q8: the pass takes int8 group-quantized weights, and only those (l2z_verify_q8)
int check_target(const char *fn, const l2z_config *config, l2z_runstate *s, const l2z_weights *w, bool q8 = false)
{
    L2Z_CHECK(s->comm == nullptr && s->sh.world == 1, L2Z_ERR_INVALID, "%s: the runstate is a shard", fn);
    if (!q8) return check_targets(fn, config, 1, &s, w);
    L2Z_TRY(check_q8_step(fn, "l2z_verify and l2z_verify_sample", s, w));
    return check_pair(config, s, w, false, true);
}

// ---- what the paths share after the checks ----

int verify_scratch(l2z_runstate *s0, bool sampled)
{
    L2Z_HIP(hipSetDevice(s0->device));
    L2Z_TRY(batch_alloc(s0));
    L2Z_TRY(verify_alloc(s0));
    if (sampled) L2Z_TRY(sample_alloc(s0));
    return L2Z_OK;
}

template <class A> A verify_attention_args(const l2z_config &c, const BatchScratch *b)
{
    A a = attention_args<A>(c, b);
    a.part_o = b->v_part_o; a.part_ml = b->v_part_ml; a.seg_cap = b->v_seg_cap;
    return a;
}

// the rows' next ids -> b->d_vout[0 .. rows): the sampler's draws if the pass is sampled, else the argmax of each row
int verify_ids(BatchScratch *b, bool sampled, int vocab, int rows, hipStream_t st)
{
    if (sampled)
        L2Z_HIP(sample_rows(b, vocab, b->d_vout, rows, st));
    else
        L2Z_HIP(launch_verify_argmax(b->v_logits, vocab, b->d_vout, rows, st));
    return L2Z_OK;
}

// after a pass: l2z_argmax scans the logits the verdict copied into s; rows: what s's own matrix holds for
// l2z_verify_logits_read
void verify_done(l2z_runstate *s, int rows)
{
    logits_whole(s, s->host_pos);  // (the caller moves the position once it has read the verdict)
    if (s->bt != nullptr) s->bt->v_rows = rows;
    wide_verify_forget(s);
}

// ---- l2z_verify, l2z_verify_sample: n consecutive positions of ONE sequence in one sweep ----

// The checks, then the table, the pass, the verdict and its copy back on s's stream; no sync.  q8: the step on int8
// group-quantized weights (batch_step's other form); everything around it is the same.
int verify_enqueue(const char *fn, const int32_t *tokens, int n, int pos0, const VerifyDraw &draw, const l2z_config *config,
                   l2z_runstate *s, const l2z_weights *w, bool q8)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && config != nullptr && s != nullptr && w != nullptr, L2Z_ERR_INVALID, "%s: null argument",
              fn);
    L2Z_CHECK(n >= 1 && n <= kBatchMax, L2Z_ERR_INVALID, "%s: n_tokens = %d outside [1, %d]", fn, n, kBatchMax);
    L2Z_TRY(check_target(fn, config, s, w, q8));
    L2Z_TRY(check_positions(fn, "", "positions", pos0, n, config->seq_len));
    L2Z_TRY(check_tokens(fn, "", tokens, n, config->vocab_size));
    if (draw.sampled()) L2Z_TRY(check_coins(fn, draw.coins, 0, n));
    L2Z_TRY(verify_scratch(s, draw.sampled()));
    if (q8) L2Z_TRY(q8_batch_alloc(s, w->q8_gs));
    BatchScratch *b = s->bt;
    const int vocab = config->vocab_size;
    BatchTable t = {};
    for (int i = 0; i < n; i++) {
        t.tokens[i] = tokens[i];
        t.pos[i] = pos0 + i;
        t.kc[i] = s->key_cache;
        t.vc[i] = s->value_cache;
        t.logits[i] = b->v_logits + (size_t)i * vocab;
        if (draw.sampled()) {
            t.temperature[i] = draw.temperature;
            t.top_p[i] = draw.top_p;
            t.coin[i] = draw.coins[i];
        }
    }
    hipStream_t st = s->stream;
    L2Z_TRY(upload_table(b, t, st));
    VerifyAttnArgs a = verify_attention_args<VerifyAttnArgs>(*config, b);
    a.pos0 = pos0;
    L2Z_TRY(batch_step(n, *config, s, w, b, [&](size_t layer_off) -> int {
        a.kc = s->key_cache + layer_off; a.vc = s->value_cache + layer_off;
        L2Z_HIP(launch_verify_attention(a, n, st));
        L2Z_HIP(launch_verify_combine(a, n, st));
        return L2Z_OK;
    }));
    L2Z_TRY(verify_ids(b, draw.sampled(), vocab, n, st));
    L2Z_HIP(launch_verify_accept(b->d_tab, b->v_logits, vocab, b->d_vout, s->logits, n, st));
    L2Z_HIP(hipMemcpyAsync(b->h_vout, b->d_vout, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, st));
    verify_done(s, n);
    return L2Z_OK;
}

// The call under either name: l2z_verify is the draw at temperature 0
int verify_call(const char *fn, const int32_t *tokens, int n, int pos0, const VerifyDraw &draw, const l2z_config *config,
                l2z_runstate *s, const l2z_weights *w, int32_t *out_next, int *out_accepted, bool q8 = false)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out_next != nullptr && out_accepted != nullptr, L2Z_ERR_INVALID, "%s: null argument", fn);
    L2Z_TRY(check_draw(fn, -1, draw.temperature, draw.top_p, draw.coins));
    L2Z_TRY(verify_enqueue(fn, tokens, n, pos0, draw, config, s, w, q8));
    BatchScratch *b = s->bt;
    L2Z_HIP(hipStreamSynchronize(s->stream));
    memcpy(out_next, b->h_vout, (size_t)n * 4);
    *out_accepted = b->h_vout[n];
    s->host_pos = pos0 + *out_accepted + 1;
    return L2Z_OK;
}

// Testing support: one call, then `iters` passes back to back (the rows' ids, the verdict and its copy included, no sync),
// timed by device events on the runstate's stream.  The passes rewrite the same KV rows.
int verify_time(const char *fn, const int32_t *tokens, int n, int pos0, const VerifyDraw &draw, const l2z_config *config,
                l2z_runstate *s, const l2z_weights *w, int iters, double *out_ms, bool q8 = false)
{
    L2Z_CHECK(iters >= 1 && out_ms != nullptr, L2Z_ERR_INVALID, "%s_time: bad arguments", fn);
    int32_t next[kBatchMax];
    int acc = 0;
    L2Z_TRY(verify_call(fn, tokens, n, pos0, draw, config, s, w, next, &acc, q8));  // validates, allocates
    return timed_loop(s->stream, iters, out_ms, [&] { return verify_enqueue(fn, tokens, n, pos0, draw, config, s, w, q8); });
}

}  // namespace
}  // namespace l2z

using namespace l2z;

extern "C" int l2z_verify(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
                          const l2z_weights *w, int32_t *out_next, int *out_accepted)
{
    return verify_call("l2z_verify", tokens, n_tokens, pos0, kGreedy, config, s, w, out_next, out_accepted);
}

extern "C" int l2z_verify_sample(const int32_t *tokens, int n_tokens, int pos0, float temperature, float top_p,
                                 const float *coins, const l2z_config *config, l2z_runstate *s, const l2z_weights *w,
                                 int32_t *out_next, int *out_accepted)
{
    return verify_call("l2z_verify_sample", tokens, n_tokens, pos0, VerifyDraw{temperature, top_p, coins}, config, s, w, out_next,
                       out_accepted);
}

// scripts/verify_bench.py
extern "C" int l2z_verify_time(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
                               const l2z_weights *w, int iters, double *out_ms)
{
    return verify_time("l2z_verify", tokens, n_tokens, pos0, kGreedy, config, s, w, iters, out_ms);
}

// scripts/verify_sample_bench.py
extern "C" int l2z_verify_sample_time(const int32_t *tokens, int n_tokens, int pos0, float temperature, float top_p,
                                      const float *coins, const l2z_config *config, l2z_runstate *s, const l2z_weights *w,
                                      int iters, double *out_ms)
{
    return verify_time("l2z_verify_sample", tokens, n_tokens, pos0, VerifyDraw{temperature, top_p, coins}, config, s, w, iters,
                       out_ms);
}

// PREVIEW (include/llama2_hip_test.h): l2z_verify's contract -- temperature 0, coins NULL -- or l2z_verify_sample's on int8
// group-quantized weights
extern "C" int l2z_verify_q8(const int32_t *tokens, int n_tokens, int pos0, float temperature, float top_p, const float *coins,
                             const l2z_config *config, l2z_runstate *s, const l2z_weights *w, int32_t *out_next,
                             int *out_accepted)
{
    return verify_call("l2z_verify_q8", tokens, n_tokens, pos0, VerifyDraw{temperature, top_p, coins}, config, s, w, out_next,
                       out_accepted, true);
}

// scripts/q8_batch_bench.py
extern "C" int l2z_verify_q8_time(const int32_t *tokens, int n_tokens, int pos0, float temperature, float top_p,
                                  const float *coins, const l2z_config *config, l2z_runstate *s, const l2z_weights *w, int iters,
                                  double *out_ms)
{
    return verify_time("l2z_verify_q8", tokens, n_tokens, pos0, VerifyDraw{temperature, top_p, coins}, config, s, w, iters,
                       out_ms, true);
}

// Testing support (include/llama2_hip_test.h): row `row` of the last l2z_verify call's logits matrix
extern "C" int l2z_verify_logits_read(l2z_runstate *s, int row, float *out)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(s != nullptr && out != nullptr, L2Z_ERR_INVALID, "l2z_verify_logits_read: null argument");
    if (const float *wide = wide_verify_row(s, row)) {  // the last verify call was l2z_verify_wide with s as states[0]
        L2Z_HIP(hipSetDevice(s->device));
        L2Z_HIP(hipMemcpyAsync(out, wide, (size_t)s->cfg.vocab_size * 4, hipMemcpyDeviceToHost, s->stream));
        L2Z_HIP(hipStreamSynchronize(s->stream));
        return L2Z_OK;
    }
    L2Z_CHECK(s->bt != nullptr && s->bt->v_logits != nullptr && row >= 0 && row < s->bt->v_rows, L2Z_ERR_STATE,
              "l2z_verify_logits_read: row %d is not a row of this runstate's last l2z_verify call", row);
    L2Z_HIP(hipSetDevice(s->device));
    L2Z_HIP(hipMemcpyAsync(out, s->bt->v_logits + (size_t)row * s->cfg.vocab_size, (size_t)s->cfg.vocab_size * 4,
                           hipMemcpyDeviceToHost, s->stream));
    L2Z_HIP(hipStreamSynchronize(s->stream));
    return L2Z_OK;
}

// ---- l2z_verify_batch: the verify pass for the rows of several sequences in one sweep (include/llama2_hip_test.h) ----
extern "C" int l2z_verify_batch(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                                const float *temperature, const float *top_p, const float *coins, const l2z_config *config,
                                l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next, int32_t *out_accepted)
{
    const char *fn = "l2z_verify_batch";
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && n_tokens != nullptr && pos0 != nullptr && config != nullptr && w != nullptr &&
                  out_next != nullptr && out_accepted != nullptr,
              L2Z_ERR_INVALID, "%s: null argument", fn);
    L2Z_TRY(check_states(fn, n, states, config));
    int R = 0;
    for (int j = 0; j < n; j++) {
        L2Z_CHECK(n_tokens[j] >= 1 && n_tokens[j] <= kBatchMax, L2Z_ERR_INVALID, "%s: n_tokens[%d] = %d outside [1, %d]", fn, j,
                  n_tokens[j], kBatchMax);
        R += n_tokens[j];
    }
    L2Z_CHECK(R <= kBatchMax, L2Z_ERR_INVALID, "%s: %d rows in all, above %d", fn, R, kBatchMax);
    L2Z_TRY(check_targets(fn, config, n, states, w));
    bool sampled = false;  // any sequence at temperature > 0: the rows' ids are sample_batch_kernel's
    if (temperature != nullptr) {  // l2z_verify_sample's rules, per sequence
        L2Z_CHECK(top_p != nullptr, L2Z_ERR_INVALID, "%s: top_p is NULL beside a temperature array", fn);
        for (int j = 0, r = 0; j < n; r += n_tokens[j], j++) {
            L2Z_TRY(check_draw(fn, j, temperature[j], top_p[j], coins));
            if (temperature[j] == 0.0f) continue;
            sampled = true;
            L2Z_TRY(check_coins(fn, coins, r, n_tokens[j]));
        }
    }
    for (int j = 0, r = 0; j < n; r += n_tokens[j], j++) {
        char where[32];
        snprintf(where, sizeof where, "sequence %d: ", j);
        L2Z_TRY(check_positions(fn, where, "positions", pos0[j], n_tokens[j], config->seq_len));
        L2Z_TRY(check_tokens(fn, where, tokens + r, n_tokens[j], config->vocab_size));
    }
    l2z_runstate *s0 = states[0];
    L2Z_TRY(verify_scratch(s0, sampled));
    BatchScratch *b = s0->bt;
    const int vocab = config->vocab_size;
    // ---- the step's table (a row per position) and the row groups (one per sequence) ----
    BatchTable t = {};
    VerifyGroupTable g = {};
    int segments = 1;  // the deepest group's
    for (int j = 0, r = 0; j < n; r += n_tokens[j], j++) {
        g.first[j] = r; g.count[j] = n_tokens[j]; g.pos0[j] = pos0[j];
        g.kc[j] = states[j]->key_cache; g.vc[j] = states[j]->value_cache; g.dst[j] = states[j]->logits;
        segments = std::max(segments, (pos0[j] + n_tokens[j] - 1) / kVerifySeg + 1);
        for (int i = 0; i < n_tokens[j]; i++) {
            t.tokens[r + i] = tokens[r + i];
            t.pos[r + i] = pos0[j] + i;
            t.kc[r + i] = states[j]->key_cache;
            t.vc[r + i] = states[j]->value_cache;
            t.logits[r + i] = b->v_logits + (size_t)(r + i) * vocab;
            if (sampled) {  // a temperature-0 sequence's rows are arg-maxed by the sampler's kernel: no coin is read
                t.temperature[r + i] = temperature[j];
                t.top_p[r + i] = top_p[j];
                t.coin[r + i] = temperature[j] > 0.0f ? coins[r + i] : 0.0f;
            }
        }
    }
    hipStream_t st = s0->stream;
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(upload_table(b, t, st, &g, sizeof g));
    const VerifyGroupTable *d_groups = (const VerifyGroupTable *)b->d_behind;
    VerifyBatchAttnArgs a = verify_attention_args<VerifyBatchAttnArgs>(*config, b);
    a.tab = b->d_tab; a.groups = d_groups;
    L2Z_TRY(batch_step(R, *config, s0, w, b, [&](size_t layer_off) -> int {
        a.layer_off = layer_off;
        L2Z_HIP(launch_verify_batch_attention(a, n, segments, st));
        L2Z_HIP(launch_verify_batch_combine(a, R, st));
        return L2Z_OK;
    }));
    L2Z_TRY(verify_ids(b, sampled, vocab, R, st));
    L2Z_HIP(launch_verify_batch_accept(b->d_tab, d_groups, b->v_logits, vocab, b->d_vout, R, n, st));
    L2Z_HIP(hipMemcpyAsync(b->h_vout, b->d_vout, (size_t)(R + n) * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(release_streams(b, n, states));
    for (int j = 0; j < n; j++) verify_done(states[j], j == 0 ? R : 0);  // the matrix is states[0]'s
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_next, b->h_vout, (size_t)R * 4);
    for (int j = 0; j < n; j++) {
        out_accepted[j] = b->h_vout[R + j];
        states[j]->host_pos = pos0[j] + out_accepted[j] + 1;
    }
    return L2Z_OK;
}

// ---- l2z_verify_tree: the verify pass for a TREE of guesses on one sequence (include/llama2_hip_test.h) ----
namespace l2z {
namespace {

// The checks, then the tables, the pass, the verdict, the compaction and the verdict's copy back on s's stream; no sync.
int verify_tree_enqueue(const int32_t *tokens, const int32_t *parent, int n, int pos0, float temperature, float top_p,
                        const float *coins, const l2z_config *config, l2z_runstate *s, const l2z_weights *w)
{
    const char *fn = "l2z_verify_tree";
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && parent != nullptr && config != nullptr && s != nullptr && w != nullptr, L2Z_ERR_INVALID,
              "%s: null argument", fn);
    L2Z_CHECK(n >= 1 && n <= kBatchMax, L2Z_ERR_INVALID, "%s: n_nodes = %d outside [1, %d]", fn, n, kBatchMax);
    L2Z_CHECK(parent[0] == -1, L2Z_ERR_INVALID, "%s: parent[0] = %d (the root's is -1)", fn, parent[0]);
    VerifyTreeTable g = {};
    int max_depth = 0;
    g.parent[0] = -1;
    g.below[0] = 1u;
    g.level[0] = 1u;
    for (int i = 1; i < n; i++) {
        L2Z_CHECK(parent[i] >= 0 && parent[i] < i, L2Z_ERR_INVALID, "%s: parent[%d] = %d outside [0, %d)", fn, i, parent[i], i);
        g.parent[i] = parent[i];
        g.depth[i] = g.depth[parent[i]] + 1;
        g.level[g.depth[i]] |= 1u << i;
        for (int j = i; j >= 0; j = g.parent[j]) g.below[j] |= 1u << i;
        max_depth = std::max(max_depth, g.depth[i]);
    }
    for (int i = 1; i < n; i++)
        for (int j = 1; j < i; j++)
            L2Z_CHECK(parent[i] != parent[j] || tokens[i] != tokens[j], L2Z_ERR_INVALID,
                      "%s: nodes %d and %d are siblings with one token (%d)", fn, j, i, tokens[i]);
    L2Z_TRY(check_target(fn, config, s, w));
    const VerifyDraw draw = {temperature, top_p, coins};
    // l2z_verify_sample's rules under ITS name, as these messages have always read: the one fn that is not the caller's
    L2Z_TRY(check_draw("l2z_verify_sample", -1, temperature, top_p, coins));
    if (draw.sampled()) L2Z_TRY(check_coins(fn, coins, 0, max_depth + 1));  // one coin per depth
    L2Z_TRY(check_positions(fn, "", "cache rows", pos0, n, config->seq_len));
    L2Z_TRY(check_tokens(fn, "", tokens, n, config->vocab_size));
    L2Z_TRY(verify_scratch(s, draw.sampled()));
    BatchScratch *b = s->bt;
    const int vocab = config->vocab_size;
    const size_t hs = (size_t)config->dim / config->n_heads;
    BatchTable t = {};
    for (int i = 0; i < n; i++) {
        t.tokens[i] = tokens[i];
        t.pos[i] = pos0 + g.depth[i];  // RoPE and the cache index of the step's epilogue ...
        t.kc[i] = s->key_cache + (size_t)(i - g.depth[i]) * hs;  // ... which so lands in physical row pos0 + i (i >= depth)
        t.vc[i] = s->value_cache + (size_t)(i - g.depth[i]) * hs;
        t.logits[i] = b->v_logits + (size_t)i * vocab;
        if (draw.sampled()) {
            t.temperature[i] = temperature;
            t.top_p[i] = top_p;
            t.coin[i] = coins[g.depth[i]];
        }
    }
    hipStream_t st = s->stream;
    L2Z_TRY(upload_table(b, t, st, &g, sizeof g));
    VerifyTreeAttnArgs a = verify_attention_args<VerifyTreeAttnArgs>(*config, b);
    a.tree = (const VerifyTreeTable *)b->d_behind; a.pos0 = pos0;
    L2Z_TRY(batch_step(n, *config, s, w, b, [&](size_t layer_off) -> int {
        a.kc = s->key_cache + layer_off; a.vc = s->value_cache + layer_off;
        L2Z_HIP(launch_verify_tree_attention(a, n, max_depth, st));
        L2Z_HIP(launch_verify_tree_combine(a, n, max_depth, st));
        return L2Z_OK;
    }));
    L2Z_TRY(verify_ids(b, draw.sampled(), vocab, n, st));
    L2Z_HIP(launch_verify_tree_accept(b->d_tab, a.tree, b->v_logits, vocab, b->d_vout, s->logits, n, st));
    L2Z_HIP(launch_verify_tree_compact(s->key_cache, s->value_cache, b->d_vout, n, pos0, (int)hs, (size_t)config->seq_len * hs,
                                       config->n_layers, config->n_kv_heads, st));
    L2Z_HIP(hipMemcpyAsync(b->h_vout, b->d_vout, (size_t)(2 * n + 1) * 4, hipMemcpyDeviceToHost, st));
    verify_done(s, n);
    return L2Z_OK;
}

}  // namespace
}  // namespace l2z

extern "C" int l2z_verify_tree(const int32_t *tokens, const int32_t *parent, int n_nodes, int pos0, float temperature,
                               float top_p, const float *coins, const l2z_config *config, l2z_runstate *s,
                               const l2z_weights *w, int32_t *out_next, int32_t *out_path, int *out_accepted)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out_next != nullptr && out_path != nullptr && out_accepted != nullptr, L2Z_ERR_INVALID,
              "l2z_verify_tree: null argument");
    L2Z_TRY(verify_tree_enqueue(tokens, parent, n_nodes, pos0, temperature, top_p, coins, config, s, w));
    BatchScratch *b = s->bt;
    L2Z_HIP(hipStreamSynchronize(s->stream));
    const int a = b->h_vout[n_nodes];
    memcpy(out_next, b->h_vout, (size_t)n_nodes * 4);
    memcpy(out_path, b->h_vout + n_nodes + 1, (size_t)(a + 1) * 4);
    *out_accepted = a;
    s->host_pos = pos0 + a + 1;
    return L2Z_OK;
}

// Testing support: l2z_verify_time for a tree (scripts/verify_tree_bench.py): one l2z_verify_tree call, then `iters` passes
// back to back (verdict, compaction and the copy included, no sync).  The passes rewrite the same KV rows; a pass whose
// verdict moved rows leaves the next one the same inputs, since every node's row is written again before it is read.
extern "C" int l2z_verify_tree_time(const int32_t *tokens, const int32_t *parent, int n_nodes, int pos0, float temperature,
                                    float top_p, const float *coins, const l2z_config *config, l2z_runstate *s,
                                    const l2z_weights *w, int iters, double *out_ms)
{
    L2Z_CHECK(iters >= 1 && out_ms != nullptr, L2Z_ERR_INVALID, "l2z_verify_tree_time: bad arguments");
    int32_t next[kBatchMax], path[kBatchMax];
    int acc = 0;
    L2Z_TRY(l2z_verify_tree(tokens, parent, n_nodes, pos0, temperature, top_p, coins, config, s, w, next, path, &acc));
    return timed_loop(s->stream, iters, out_ms, [&] {
        return verify_tree_enqueue(tokens, parent, n_nodes, pos0, temperature, top_p, coins, config, s, w);
    });
}
