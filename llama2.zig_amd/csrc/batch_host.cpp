// batch_host.cpp -- host side of the batched decode step (l2z_transformer_batch, l2z_argmax_batch): up to
// L2Z_BATCH_MAX independent sequences advanced by one token with one sweep of the weights.  Kernels: the short-prompt
// GEMM forms with per-row epilogues (prefill_skinny.hip, G_*_ROWS) and batch_decode.hip.  Also what a batch of samples
// needs around the step: the on-device sampler l2z_sample_batch (sample_batch.hip) and the prompt copy
// l2z_runstate_fork.  The step itself (batch_step) takes a layer's attention from its caller: the verify family
// (verify_host.cpp) runs it with attention forms of its own; on int8 group-quantized weights it is q8_host.cpp's.  batch_host.h: what the host files share -- its argument
// rules, stream hand-overs and allocation helper are defined here.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "batch_host.h"
#include "prefill_common.h"

static_assert(l2z::kBatchMax == L2Z_BATCH_MAX, "include/llama2_hip.h L2Z_BATCH_MAX");

namespace l2z {

void batch_free(l2z_runstate *s)
{
    BatchScratch *b = s->bt;
    if (b == nullptr) return;
    void *ptrs[] = {b->x, b->xn, b->q, b->att, b->h1, b->scores, b->d_tab, b->d_tokens_out, b->smp,
                    b->v_logits, b->v_part_o, b->v_part_ml, b->d_vout, b->q8_xq, b->q8_xs};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (b->h_tab) (void)hipHostFree(b->h_tab);
    if (b->h_tokens_out) (void)hipHostFree(b->h_tokens_out);
    if (b->h_vout) (void)hipHostFree(b->h_vout);
    for (hipEvent_t e : b->ev_in)
        if (e) (void)hipEventDestroy(e);
    if (b->ev_done) (void)hipEventDestroy(b->ev_done);
    if (b->ev_upload) (void)hipEventDestroy(b->ev_upload);
    delete b;
    s->bt = nullptr;
}

namespace {

// what follows the step's table in its allocations: the row groups of l2z_verify_batch or the tree of l2z_verify_tree
constexpr size_t kTabExtra = std::max(sizeof(VerifyGroupTable), sizeof(VerifyTreeTable));

// Row pitch of the activation matrices the GEMMs read: rounded up to 256 floats, at least 768, the pad columns zero and
// never written (the short-prompt forms multiply whole 256-k stages, at least three: prefill_common.h pad_k)
int bt_ld(int n)
{
    const int r = (n + 255) / 256 * 256;
    return r < 768 ? 768 : r;
}

}  // namespace

int batch_alloc(l2z_runstate *s)
{
    if (s->bt != nullptr) return L2Z_OK;
    const l2z_config &c = s->cfg;
    BatchScratch *b = new BatchScratch();
    s->bt = b;  // freed with the runstate whatever happens below
    b->ld_xn = bt_ld(c.dim); b->ld_att = bt_ld(c.dim); b->ld_h1 = bt_ld(c.hidden_dim);
    const size_t R = kBatchMax;
    L2Z_TRY(alloc_all("batched step scratch",
                      {{(void **)&b->x, R * c.dim * 4}, {(void **)&b->xn, R * b->ld_xn * 4}, {(void **)&b->q, R * c.dim * 4},
                       {(void **)&b->att, R * b->ld_att * 4}, {(void **)&b->h1, R * b->ld_h1 * 4},
                       {(void **)&b->scores, R * (size_t)c.n_heads * c.seq_len * 4},
                       {(void **)&b->d_tab, sizeof(BatchTable) + kTabExtra}, {(void **)&b->d_tokens_out, R * 4}}));
    L2Z_HIP(hipHostMalloc((void **)&b->h_tab, sizeof(BatchTable) + kTabExtra, hipHostMallocDefault));
    b->d_behind = b->d_tab + 1;
    b->h_behind = b->h_tab + 1;
    L2Z_HIP(hipHostMalloc((void **)&b->h_tokens_out, R * 4, hipHostMallocDefault));
    for (hipEvent_t &e : b->ev_in) L2Z_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    L2Z_HIP(hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming));
    L2Z_HIP(hipEventCreateWithFlags(&b->ev_upload, hipEventDisableTiming));
    // the pad columns are multiplied against whatever follows a W row: zeros, once
    L2Z_HIP(hipMemset(b->xn, 0, R * b->ld_xn * 4));
    L2Z_HIP(hipMemset(b->att, 0, R * b->ld_att * 4));
    L2Z_HIP(hipMemset(b->h1, 0, R * b->ld_h1 * 4));
    return L2Z_OK;
}

int sample_alloc(l2z_runstate *s)
{
    BatchScratch *b = s->bt;
    if (b->smp != nullptr) return L2Z_OK;
    const size_t stride = sample_scratch_floats(s->cfg.vocab_size);
    L2Z_TRY(alloc_all("l2z_sample_batch scratch", {{(void **)&b->smp, kBatchMax * stride * 4}}));
    b->smp_stride = stride;
    return L2Z_OK;
}

int verify_alloc(l2z_runstate *s)
{
    BatchScratch *b = s->bt;
    if (b->v_logits != nullptr && b->v_part_o != nullptr && b->v_part_ml != nullptr && b->d_vout != nullptr &&
        b->h_vout != nullptr)
        return L2Z_OK;
    const l2z_config &c = s->cfg;
    const size_t R = kBatchMax, segs = (size_t)verify_segments(c.seq_len), hs = (size_t)c.dim / c.n_heads;
    // (a call that failed part of the way left some of them: those stay)
    L2Z_TRY(alloc_all("l2z_verify scratch", {{(void **)&b->v_logits, R * (size_t)c.vocab_size * 4},
                                             {(void **)&b->v_part_o, R * c.n_heads * segs * hs * 4},
                                             {(void **)&b->v_part_ml, R * c.n_heads * segs * 2 * 4},
                                             {(void **)&b->d_vout, 3 * R * 4}}));
    if (b->h_vout == nullptr) L2Z_HIP(hipHostMalloc((void **)&b->h_vout, 3 * R * 4, hipHostMallocDefault));
    b->v_seg_cap = (int)segs;
    return L2Z_OK;
}

int q8_batch_alloc(l2z_runstate *s, int gs)
{
    BatchScratch *b = s->bt;
    if (b->q8_xq != nullptr && b->q8_xs != nullptr && b->q8_gs == gs) return L2Z_OK;
    if (b->q8_gs != gs && (b->q8_xq != nullptr || b->q8_xs != nullptr)) {   // another group size: other scale rows
        L2Z_HIP(hipStreamSynchronize(s->stream));
        if (b->q8_xq) { (void)hipFree(b->q8_xq); b->q8_xq = nullptr; }
        if (b->q8_xs) { (void)hipFree(b->q8_xs); b->q8_xs = nullptr; }
    }
    b->q8_gs = gs;
    const size_t R = kBatchMax, widest = (size_t)std::max(s->cfg.dim, s->cfg.hidden_dim);
    return alloc_all("batched q8 step scratch", {{(void **)&b->q8_xq, R * widest}, {(void **)&b->q8_xs, R * (widest / (size_t)gs) * 4}});
}

int check_q8_step(const char *fn, const char *f32_entry, const l2z_runstate *s0, const l2z_weights *w)
{
    L2Z_CHECK(w->is_q8(), L2Z_ERR_INVALID,
              "%s: takes int8 group-quantized weights (l2z_weights_init_q8); f32 and packed weights go to %s", fn, f32_entry);
    L2Z_CHECK(s0->sh.hs % 4 == 0 && s0->sh.hs <= 256, L2Z_ERR_INVALID,
              "%s: needs a head_size that is a multiple of 4, at most 256", fn);
    L2Z_CHECK(s0->cfg.vocab_size % 4 == 0, L2Z_ERR_INVALID, "%s: needs a vocab_size that is a multiple of 4 (it is %d)", fn,
              s0->cfg.vocab_size);
    return L2Z_OK;
}

int alloc_all(const char *what, std::initializer_list<DeviceBuf> want)
{
    for (const DeviceBuf &w : want) {
        if (*w.p != nullptr || w.bytes == 0) continue;
        const hipError_t e = hipMalloc(w.p, w.bytes);
        if (e != hipSuccess) {
            *w.p = nullptr;
            set_error("%s allocation (%zu bytes) failed: %s", what, w.bytes, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? L2Z_ERR_OOM : L2Z_ERR_HIP;
        }
    }
    return L2Z_OK;
}

int no_device_check()
{
    int nd = 0;
    const hipError_t e = hipGetDeviceCount(&nd);
    L2Z_CHECK(e == hipSuccess && nd > 0, L2Z_ERR_NO_DEVICE, "no HIP device available; this library has no CPU fallback");
    return L2Z_OK;
}

int check_states(const char *fn, int n, l2z_runstate *const *states, const l2z_config *c, int n_max)
{
    L2Z_CHECK(n >= 1 && n <= n_max, L2Z_ERR_INVALID, "%s: n = %d outside [1, %d]", fn, n, n_max);
    L2Z_CHECK(states != nullptr, L2Z_ERR_INVALID, "%s: null runstate array", fn);
    for (int i = 0; i < n; i++) {
        const l2z_runstate *s = states[i];
        L2Z_CHECK(s != nullptr, L2Z_ERR_INVALID, "%s: states[%d] is null", fn, i);
        for (int j = 0; j < i; j++)
            L2Z_CHECK(states[j] != s, L2Z_ERR_INVALID, "%s: states[%d] and states[%d] are the same runstate", fn, j, i);
        L2Z_CHECK(s->comm == nullptr && s->sh.world == 1, L2Z_ERR_INVALID, "%s: states[%d] is a shard (shard groups are not batched)", fn, i);
        L2Z_CHECK(memcmp(c != nullptr ? c : &states[0]->cfg, &s->cfg, sizeof(l2z_config)) == 0, L2Z_ERR_INVALID,
                  "%s: states[%d] was made with another config", fn, i);
        L2Z_CHECK(s->device == states[0]->device, L2Z_ERR_INVALID, "%s: states[%d] is on device %d, states[0] on %d", fn, i,
                  s->device, states[0]->device);
    }
    return L2Z_OK;
}

int check_positions(const char *fn, const char *where, const char *what, int pos0, int n, int seq_len)
{
    L2Z_CHECK(pos0 >= 0 && pos0 <= seq_len - n, L2Z_ERR_STATE, "%s: %s%s %d .. %lld outside [0, %d)", fn, where, what, pos0,
              (long long)pos0 + n - 1, seq_len);
    return L2Z_OK;
}

int check_tokens(const char *fn, const char *where, const int32_t *tokens, int n, int vocab, int first)
{
    for (int i = 0; i < n; i++)
        L2Z_CHECK(tokens[i] >= 0 && tokens[i] < vocab, L2Z_ERR_STATE, "%s: %stokens[%d] = %d out of vocabulary", fn, where,
                  first + i, tokens[i]);
    return L2Z_OK;
}

int check_row(const char *fn, int i, int32_t token, int32_t pos, int n_pos, const l2z_config &c)
{
    char what[24];
    snprintf(what, sizeof what, "pos[%d] =", i);
    L2Z_TRY(check_positions(fn, "", what, pos, n_pos, c.seq_len));
    return check_tokens(fn, "", &token, 1, c.vocab_size, i);
}

int check_draw(const char *fn, int seq, float temperature, float top_p, const float *coins)
{
    char idx[16] = "";
    if (seq >= 0) snprintf(idx, sizeof idx, "[%d]", seq);
    L2Z_CHECK(std::isfinite(temperature) && temperature >= 0.0f, L2Z_ERR_INVALID, "%s: temperature%s = %g (finite, >= 0)", fn, idx,
              (double)temperature);
    L2Z_CHECK(top_p >= 0.0f && top_p <= 1.0f, L2Z_ERR_INVALID, "%s: top_p%s = %g outside [0, 1]", fn, idx, (double)top_p);
    L2Z_CHECK(temperature == 0.0f || coins != nullptr, L2Z_ERR_INVALID, "%s: coins is NULL at temperature%s%s%g", fn, idx,
              seq >= 0 ? " = " : " ", (double)temperature);
    return L2Z_OK;
}

int check_coins(const char *fn, const float *coins, int first, int count, int stride)
{
    for (long long i = first; i < first + (long long)count * stride; i += stride)
        L2Z_CHECK(coins[i] >= 0.0f && coins[i] < 1.0f, L2Z_ERR_INVALID, "%s: coins[%lld] = %g outside [0, 1)", fn, i, (double)coins[i]);
    return L2Z_OK;
}

int check_ragged_call(const RaggedCall &c, RaggedTotals *t)
{
    const char *fn = c.fn;
    L2Z_TRY(no_device_check());
    L2Z_CHECK(c.tokens != nullptr && c.pos0 != nullptr && c.config != nullptr && c.w != nullptr, L2Z_ERR_INVALID, "%s: null argument", fn);
    L2Z_TRY(check_states(fn, c.n, c.states, c.config, c.max_seq));
    L2Z_TRY(kv_check_kind(fn, c.n, c.states));
    auto rows_of = [&c](int j) { return c.n_tokens != nullptr ? c.n_tokens[j] : 1; };
    long long rows = 0;   // (no sum of n counts overflows it)
    *t = {};
    for (int j = 0; j < c.n; j++) {
        L2Z_CHECK(rows_of(j) >= 1, L2Z_ERR_INVALID, "%s: n_tokens[%d] = %d (at least 1)", fn, j, rows_of(j));
        L2Z_CHECK(c.max_seq_rows == 0 || rows_of(j) <= c.max_seq_rows, L2Z_ERR_INVALID, "%s: n_tokens[%d] = %d above %d", fn, j,
                  rows_of(j), c.max_seq_rows);
        rows += rows_of(j);
        L2Z_CHECK(c.max_rows == 0 || rows <= c.max_rows, L2Z_ERR_INVALID, "%s: more than %d rows in all", fn, c.max_rows);
        t->longest = std::max(t->longest, rows_of(j));
    }
    for (int j = 0; j < c.n; j++) L2Z_TRY(check_pair(c.config, c.states[j], c.w, true));
    L2Z_TRY(prefill_check(c.config, c.states[0]));
    if (c.temperature != nullptr) {   // l2z_sample_batch's rules for every sequence; a greedy one's coins are not read
        L2Z_CHECK(c.top_p != nullptr, L2Z_ERR_INVALID, "%s: top_p is NULL beside a temperature array", fn);
        for (int j = 0, r = 0; j < c.n; r += rows_of(j), j++) {
            L2Z_TRY(check_draw(fn, j, c.temperature[j], c.top_p[j], c.coins));
            if (c.temperature[j] == 0.0f) continue;
            t->sampled = true;
            L2Z_TRY(c.coins_per_step ? check_coins(fn, c.coins, j, c.n_steps, c.n) : check_coins(fn, c.coins, r, rows_of(j)));
        }
    }
    for (int j = 0, r = 0; j < c.n; r += rows_of(j), j++) {   // (a sequence that passed fits the cache: r cannot overflow)
        char where[32];
        snprintf(where, sizeof where, "sequence %d: ", j);
        L2Z_TRY(check_positions(fn, where, "positions", c.pos0[j], rows_of(j) + c.n_steps - 1, c.config->seq_len));
        L2Z_TRY(check_tokens(fn, where, c.tokens + r, rows_of(j), c.config->vocab_size));
        t->deepest = std::max(t->deepest, c.pos0[j] + rows_of(j) - 1);
    }
    t->R = (int)rows;
    return L2Z_OK;
}

int upload_table(BatchScratch *b, const BatchTable &t, hipStream_t st, const void *behind, size_t behind_bytes)
{
    L2Z_HIP(hipEventSynchronize(b->ev_upload));
    memcpy(b->h_tab, &t, sizeof t);
    if (behind_bytes != 0) memcpy(b->h_behind, behind, behind_bytes);
    L2Z_HIP(hipMemcpyAsync(b->d_tab, b->h_tab, sizeof t + behind_bytes, hipMemcpyHostToDevice, st));
    L2Z_HIP(hipEventRecord(b->ev_upload, st));
    return L2Z_OK;
}

// Every product is the one-tile short-prompt form at P = n whatever n is (launch_batch_skinny): a row's bits do not depend
// on n, on the other rows, or on its place in the batch.
int batch_step(int n, const l2z_config &c, l2z_runstate *s0, const l2z_weights *w, BatchScratch *b, LayerAttention attention)
{
    if (w->is_q8()) return batch_step_q8(n, c, s0, w, b, attention);
    hipStream_t st = s0->stream;
    const int dim = c.dim, hid = c.hidden_dim, hs = dim / c.n_heads, kvd = hs * c.n_kv_heads;
    const BatchTable *tab = b->d_tab;
    L2Z_HIP(launch_prefill_embed(b->x, w->tok_emb, tab->tokens, dim, n, st));  // :295
    for (int l = 0; l < c.n_layers; l++) {
        const size_t layer_off = (size_t)l * c.seq_len * kvd;
        L2Z_HIP(launch_prefill_rmsnorm(b->xn, b->ld_xn, b->x, w->rms_att + (size_t)l * dim, dim, n, st));  // :305
        {   // q (:308-351): RoPE at each row's own position
            GemmArgs a = gemm(b->xn, b->ld_xn, w->wq + (size_t)l * dim * dim, dim, dim, dim, n);
            a.out = b->q; a.ldo = dim; a.rope = s0->rope; a.head_size = hs; a.row_pos = tab->pos;
            L2Z_HIP(launch_batch_skinny(G_ROPE_ROWS, a, st));
        }
        {   // k | v (:354-358) into each row's own caches, row = its position
            GemmArgs a = gemm(b->xn, b->ld_xn, w->wk + (size_t)l * kvd * dim, dim, kvd, dim, n);
            a.w2 = w->wv + (size_t)l * kvd * dim;
            a.rope = s0->rope; a.head_size = hs; a.ldkv = kvd; a.kv_head_stride = (size_t)c.seq_len * hs;
            a.row_pos = tab->pos; a.row_kc = tab->kc; a.row_vc = tab->vc; a.layer_off = layer_off;
            L2Z_HIP(launch_batch_skinny(G_QKV_ROWS, a, st));
        }
        L2Z_TRY(attention(layer_off));  // :361-389
        {   // :392-395
            GemmArgs a = gemm(b->att, b->ld_att, w->wo + (size_t)l * dim * dim, dim, dim, dim, n);
            a.out = b->x; a.ldo = dim; a.res = b->x; a.ldres = dim;
            L2Z_HIP(launch_batch_skinny(G_RESID, a, st));
        }
        L2Z_HIP(launch_prefill_rmsnorm(b->xn, b->ld_xn, b->x, w->rms_ffn + (size_t)l * dim, dim, n, st));  // :398
        {   // :405-416: W1 | W3 (rows 2 dim apart in their shared slot) with silu(a) * b in the epilogue
            GemmArgs a = gemm(b->xn, b->ld_xn, w->w1 + (size_t)l * hid * 2 * dim, 2 * dim, hid, dim, n);
            a.w2 = w->w3 + (size_t)l * hid * 2 * dim;
            a.out = b->h1; a.ldo = b->ld_h1;
            L2Z_HIP(launch_batch_skinny(G_SWIGLU, a, st));
        }
        {   // :419-422
            GemmArgs a = gemm(b->h1, b->ld_h1, w->w2 + (size_t)l * dim * hid, hid, dim, hid, n);
            a.out = b->x; a.ldo = dim; a.res = b->x; a.ldres = dim;
            L2Z_HIP(launch_batch_skinny(G_RESID, a, st));
        }
    }
    L2Z_HIP(launch_prefill_rmsnorm(b->xn, b->ld_xn, b->x, w->rms_final, dim, n, st));  // :426
    {   // :429: each row's logits straight into its runstate
        GemmArgs a = gemm(b->xn, b->ld_xn, w->wcls, dim, c.vocab_size, dim, n);
        a.row_out = tab->logits;
        L2Z_HIP(launch_batch_skinny(G_OUT_ROWS, a, st));
    }
    return L2Z_OK;
}

hipError_t sample_rows(BatchScratch *b, int vocab, int *out, int n, hipStream_t st)
{
    SampleArgs a = {};
    a.tab = b->d_tab; a.scratch = b->smp; a.row_stride = b->smp_stride; a.vocab = vocab; a.out = out;
    return launch_sample_batch(a, n, st);
}

int timed_loop(hipStream_t st, int iters, double *out_ms, FnRef<int()> pass)
{
    hipEvent_t e0, e1;
    L2Z_HIP(hipEventCreate(&e0));
    L2Z_HIP(hipEventCreate(&e1));
    int rc = L2Z_OK;
    if (hipEventRecord(e0, st) != hipSuccess) rc = L2Z_ERR_HIP;
    for (int i = 0; i < iters && rc == L2Z_OK; i++) rc = pass();
    float ms = 0.0f;
    if (rc == L2Z_OK && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                         hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
        rc = L2Z_ERR_HIP;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc == L2Z_OK) *out_ms = ms / iters;
    return rc;
}

}  // namespace l2z

using namespace l2z;

namespace {

// l2z_transformer_batch (q8 false) and l2z_transformer_batch_q8 (true): one body, the weights' family apart
int transformer_batch_call(const char *fn, bool q8, int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                           l2z_runstate *const *states, const l2z_weights *w)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && pos != nullptr && config != nullptr && w != nullptr, L2Z_ERR_INVALID, "%s: null argument", fn);
    L2Z_TRY(check_states(fn, n, states, config));
    if (q8) L2Z_TRY(check_q8_step(fn, "l2z_transformer_batch", states[0], w));
    for (int i = 0; i < n; i++) {
        L2Z_TRY(check_pair(config, states[i], w, false, q8));
        L2Z_TRY(check_row(fn, i, tokens[i], pos[i], 1, *config));
    }
    if (!q8) {
        L2Z_TRY(prefill_check(config, states[0]));
        L2Z_CHECK(states[0]->sh.hs <= 256, L2Z_ERR_INVALID, "%s: head_size above 256", fn);
    }
    L2Z_HIP(hipSetDevice(states[0]->device));
    L2Z_TRY(batch_alloc(states[0]));
    if (q8) L2Z_TRY(q8_batch_alloc(states[0], w->q8_gs));
    BatchScratch *b = states[0]->bt;
    BatchTable t = {};
    for (int i = 0; i < n; i++) {
        t.tokens[i] = tokens[i];
        t.pos[i] = pos[i];
        t.kc[i] = states[i]->key_cache;
        t.vc[i] = states[i]->value_cache;
        t.logits[i] = states[i]->logits;
    }
    hipStream_t st = states[0]->stream;
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(upload_table(b, t, st));
    BatchAttnArgs a = attention_args<BatchAttnArgs>(*config, b);  // one block per (head, row), each row on its own caches
    a.scores = b->scores; a.tab = b->d_tab; a.seq_len = config->seq_len;
    L2Z_TRY(batch_step(n, *config, states[0], w, b, [&](size_t layer_off) -> int {
        a.layer_off = layer_off;
        L2Z_HIP(launch_batch_attention(a, n, st));
        return L2Z_OK;
    }));
    L2Z_TRY(release_streams(b, n, states));
    for (int i = 0; i < n; i++) logits_whole(states[i], pos[i] + 1);
    return L2Z_OK;
}

}  // namespace

extern "C" int l2z_transformer_batch(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                                     l2z_runstate *const *states, const l2z_weights *w)
{
    return transformer_batch_call("l2z_transformer_batch", false, n, tokens, pos, config, states, w);
}

// PREVIEW (include/llama2_hip_test.h): l2z_transformer_batch's contract on int8 group-quantized weights
extern "C" int l2z_transformer_batch_q8(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                                        l2z_runstate *const *states, const l2z_weights *w)
{
    return transformer_batch_call("l2z_transformer_batch_q8", true, n, tokens, pos, config, states, w);
}

extern "C" int l2z_argmax_batch(int n, l2z_runstate *const *states, int32_t *out_tokens)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out_tokens != nullptr, L2Z_ERR_INVALID, "l2z_argmax_batch: null argument");
    L2Z_TRY(check_states("l2z_argmax_batch", n, states, nullptr));
    L2Z_HIP(hipSetDevice(states[0]->device));
    L2Z_TRY(batch_alloc(states[0]));
    BatchScratch *b = states[0]->bt;
    BatchTable t = {};
    for (int i = 0; i < n; i++) t.logits[i] = states[i]->logits;
    hipStream_t st = states[0]->stream;
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(upload_table(b, t, st));
    L2Z_HIP(launch_batch_argmax(b->d_tab, states[0]->cfg.vocab_size, b->d_tokens_out, n, st));
    L2Z_HIP(hipMemcpyAsync(b->h_tokens_out, b->d_tokens_out, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_tokens, b->h_tokens_out, (size_t)n * 4);
    return L2Z_OK;
}

namespace l2z {
namespace {

// l2z_sample_batch's checks, table and launch on states[0]'s stream (no copy back)
int sample_enqueue(int n, l2z_runstate *const *states, const float *temperature, const float *top_p, const float *coins)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(temperature != nullptr && top_p != nullptr && coins != nullptr, L2Z_ERR_INVALID,
              "l2z_sample_batch: null argument");
    L2Z_TRY(check_states("l2z_sample_batch", n, states, nullptr));
    for (int i = 0; i < n; i++) {   // (a row at temperature 0 answers for its coin too)
        L2Z_TRY(check_draw("l2z_sample_batch", i, temperature[i], top_p[i], coins));
        L2Z_TRY(check_coins("l2z_sample_batch", coins, i, 1));
    }
    L2Z_HIP(hipSetDevice(states[0]->device));
    L2Z_TRY(batch_alloc(states[0]));
    L2Z_TRY(sample_alloc(states[0]));
    BatchScratch *b = states[0]->bt;
    BatchTable t = {};
    for (int i = 0; i < n; i++) {
        t.logits[i] = states[i]->logits;
        t.temperature[i] = temperature[i];
        t.top_p[i] = top_p[i];
        t.coin[i] = coins[i];
    }
    hipStream_t st = states[0]->stream;
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(upload_table(b, t, st));
    L2Z_HIP(sample_rows(b, states[0]->cfg.vocab_size, b->d_tokens_out, n, st));
    return L2Z_OK;
}

}  // namespace
}  // namespace l2z

extern "C" int l2z_sample_batch(int n, l2z_runstate *const *states, const float *temperature, const float *top_p,
                                const float *coins, int32_t *out_tokens)
{
    L2Z_CHECK(out_tokens != nullptr, L2Z_ERR_INVALID, "l2z_sample_batch: null argument");
    L2Z_TRY(sample_enqueue(n, states, temperature, top_p, coins));
    BatchScratch *b = states[0]->bt;
    hipStream_t st = states[0]->stream;
    L2Z_HIP(hipMemcpyAsync(b->h_tokens_out, b->d_tokens_out, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(release_streams(b, n, states));
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_tokens, b->h_tokens_out, (size_t)n * 4);
    return L2Z_OK;
}

extern "C" int l2z_runstate_fork(l2z_runstate *dst, const l2z_runstate *src, int n_pos)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(dst != nullptr && src != nullptr, L2Z_ERR_INVALID, "l2z_runstate_fork: null runstate");
    L2Z_CHECK(dst != src, L2Z_ERR_INVALID, "l2z_runstate_fork: dst and src are the same runstate");
    L2Z_CHECK(dst->comm == nullptr && dst->sh.world == 1 && src->comm == nullptr && src->sh.world == 1, L2Z_ERR_INVALID,
              "l2z_runstate_fork: shard runstates are not forked");
    L2Z_CHECK(memcmp(&dst->cfg, &src->cfg, sizeof(l2z_config)) == 0, L2Z_ERR_INVALID,
              "l2z_runstate_fork: dst was made with another config");
    L2Z_CHECK(dst->device == src->device, L2Z_ERR_INVALID, "l2z_runstate_fork: dst is on device %d, src on %d", dst->device,
              src->device);
    const l2z_config &c = src->cfg;
    L2Z_CHECK(n_pos >= 0 && n_pos <= c.seq_len, L2Z_ERR_STATE, "l2z_runstate_fork: n_pos = %d outside [0, %d]", n_pos,
              c.seq_len);
    L2Z_HIP(hipSetDevice(src->device));
    // ---- a paged side (include/llama2_hip_test.h l2z_kvpool): dst gives back its pages, then shares src's whole pages
    // where both draw from one pool, and attaches private ones for the rows that are copied ----
    const bool paged = dst->pool != nullptr || src->pool != nullptr;
    const int whole = dst->pool != nullptr && dst->pool == src->pool ? n_pos / kKvPage : 0;   // pages shared, not copied
    if (src->pool != nullptr)
        L2Z_CHECK(src->pool->alloc.missing(src->pg, 0, n_pos) == 0, L2Z_ERR_STATE,
                  "l2z_runstate_fork: src holds no page for some position below n_pos = %d", n_pos);
    if (dst->pool != nullptr) {
        KvPages &al = dst->pool->alloc;
        int back = 0;   // pages dst's release sets free
        for (int32_t id : dst->pg.pages) back += id >= 0 && al.refs(id) == 1;
        const int need = kv_pages_for(n_pos) - whole;
        L2Z_CHECK(need <= al.n_free() + back, L2Z_ERR_OOM, "l2z_runstate_fork: dst needs %d KV pages, the pool has %d free of %d",
                  need, al.n_free() + back, al.n_pages());
        L2Z_TRY(kv_release(dst, 0));
        al.share(dst->pg, src->pg, whole);
        (void)al.attach(dst->pg, whole * kKvPage, n_pos);   // (cannot fall short: counted above)
        dst->pages_dirty = true;
    }
    hipEvent_t ev_src = nullptr, ev_dst = nullptr;
    L2Z_HIP(hipEventCreateWithFlags(&ev_src, hipEventDisableTiming));
    int rc = L2Z_OK;
    auto hip = [&rc](hipError_t e, const char *what) {
        if (rc == L2Z_OK && e != hipSuccess) {
            set_error("l2z_runstate_fork: %s: %s", what, hipGetErrorString(e));
            rc = L2Z_ERR_HIP;
        }
    };
    hip(hipEventCreateWithFlags(&ev_dst, hipEventDisableTiming), "hipEventCreate");
    // dst's stream waits for what src's has queued (the rows and logits being copied) ...
    hip(hipEventRecord(ev_src, src->stream), "hipEventRecord");
    hip(hipStreamWaitEvent(dst->stream, ev_src, 0), "hipStreamWaitEvent");
    // ... the caches are head-major [layer][kv head][seq_len][head_size]: positions 0 .. n_pos - 1 are one
    // run of n_pos * head_size floats per (layer, kv head), seq_len * head_size floats apart
    const size_t hs = (size_t)c.dim / c.n_heads, pitch = (size_t)c.seq_len * hs * 4, width = (size_t)n_pos * hs * 4;
    const size_t rows = (size_t)c.n_layers * c.n_kv_heads;
    if (paged) {
        if (rc == L2Z_OK) rc = kv_copy_rows(dst, src, whole * kKvPage, n_pos);
    } else if (n_pos > 0 && rc == L2Z_OK) {
        hip(hipMemcpy2DAsync(dst->key_cache, pitch, src->key_cache, pitch, width, rows, hipMemcpyDeviceToDevice, dst->stream),
            "key cache copy");
        hip(hipMemcpy2DAsync(dst->value_cache, pitch, src->value_cache, pitch, width, rows, hipMemcpyDeviceToDevice,
                             dst->stream),
            "value cache copy");
    }
    if (rc == L2Z_OK)
        hip(hipMemcpyAsync(dst->logits, src->logits, (size_t)c.vocab_size * 4, hipMemcpyDeviceToDevice, dst->stream),
            "logits copy");
    // ... and src's stream waits for the copies: its next step overwrites the logits they read
    hip(hipEventRecord(ev_dst, dst->stream), "hipEventRecord");
    hip(hipStreamWaitEvent(src->stream, ev_dst, 0), "hipStreamWaitEvent");
    (void)hipEventDestroy(ev_src);  // released by the runtime once the streams are past them
    if (ev_dst) (void)hipEventDestroy(ev_dst);
    if (rc != L2Z_OK) return rc;
    logits_whole(dst, n_pos);  // (the copied logits, not dst's own classifier candidates)
    return L2Z_OK;
}

// Testing support (include/llama2_hip_test.h): place exact logits in a runstate (vocab_size floats), queued on its stream
extern "C" int l2z_logits_write(l2z_runstate *s, const float *logits)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(s != nullptr && logits != nullptr, L2Z_ERR_INVALID, "l2z_logits_write: null argument");
    L2Z_CHECK(s->comm == nullptr && s->sh.world == 1, L2Z_ERR_INVALID, "l2z_logits_write: shard runstate");
    L2Z_HIP(hipSetDevice(s->device));
    L2Z_HIP(hipMemcpyAsync(s->logits, logits, (size_t)s->cfg.vocab_size * 4, hipMemcpyHostToDevice, s->stream));
    L2Z_HIP(hipStreamSynchronize(s->stream));
    logits_whole(s, s->host_pos);
    return L2Z_OK;
}

// Testing support: `iters` l2z_sample_batch launches back to back (no copy back), timed by device events on the
// launches' stream (scripts/sample_bench.py)
extern "C" int l2z_sample_time(int n, l2z_runstate *const *states, const float *temperature, const float *top_p,
                               const float *coins, int iters, double *out_ms)
{
    L2Z_CHECK(iters >= 1 && out_ms != nullptr, L2Z_ERR_INVALID, "l2z_sample_time: bad arguments");
    L2Z_TRY(sample_enqueue(n, states, temperature, top_p, coins));  // validates, allocates, warms up
    hipStream_t st = states[0]->stream;
    BatchScratch *b = states[0]->bt;
    return timed_loop(st, iters, out_ms, [&]() -> int {
        return sample_rows(b, states[0]->cfg.vocab_size, b->d_tokens_out, n, st) == hipSuccess ? L2Z_OK : L2Z_ERR_HIP;
    });
}

namespace {

// l2z_batch_time (q8 false) and l2z_batch_q8_time (true): one body, as transformer_batch_call, whose steps it times
int batch_time_call(const char *fn, bool q8, int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                    l2z_runstate *const *states, const l2z_weights *w, int iters, double *out_ms)
{
    L2Z_CHECK(iters >= 1 && out_ms != nullptr, L2Z_ERR_INVALID, "%s: bad arguments", fn);
    const auto step = [&] {
        return transformer_batch_call(q8 ? "l2z_transformer_batch_q8" : "l2z_transformer_batch", q8, n, tokens, pos, config, states, w);
    };
    L2Z_TRY(step());  // validates, allocates
    return timed_loop(states[0]->stream, iters, out_ms, step);
}

}  // namespace

// Testing support (include/llama2_hip_test.h): `iters` batched steps back to back, timed by device events on the pass's
// stream (scripts/batch_bench.py) ...
extern "C" int l2z_batch_time(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                              l2z_runstate *const *states, const l2z_weights *w, int iters, double *out_ms)
{
    return batch_time_call("l2z_batch_time", false, n, tokens, pos, config, states, w, iters, out_ms);
}

// ... and on int8 group-quantized weights (scripts/q8_batch_bench.py)
extern "C" int l2z_batch_q8_time(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                                 l2z_runstate *const *states, const l2z_weights *w, int iters, double *out_ms)
{
    return batch_time_call("l2z_batch_q8_time", true, n, tokens, pos, config, states, w, iters, out_ms);
}
