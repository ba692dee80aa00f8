// q8_host.cpp -- host side of the multi-row passes on int8 group-quantized weights: the prompt pass l2z_prefill_q8
// (include/llama2_hip_test.h) and the batched step behind l2z_transformer_batch_q8 and l2z_verify_q8
// (batch_step_q8).  Both go through ONE layer walk (q8_layers), apart from the f32 walks
// of prefill_host.cpp and batch_step: per layer four row launches (q8_rows.hip: the group quantization of the pass's rows,
// after the rmsnorm where the decode's launch has one) and, behind the attention, three GEMM launches on the int8 matrix
// cores (q8_gemm.hip: Wo and W2 with the residual, W1 | W3 with SwiGLU).  How q | k | v, the cache rows and the attention
// output come about is the caller's: the prompt pass runs three more GEMMs into scratch, the f32 pass's RoPE + cache
// scatter over a one-sequence table and its prompt attention -- on a runstate with int8 KV rows (l2z_prefill_kv8, DESIGN.md
// 4.29) the format's scatter and the prompt attention over the int8 arrays (kv8.h) in their place -- and sends the last
// row through the decode's own classifier launch, so the runstate is left as after a decode step; the step runs
// q | k | v as one launch (q8_batch.hip), its caller's attention and the classifier through the table.  The verify pass over
// int8 KV rows (verify_kv8_pass) is the prompt pass's chunk of at most 16 rows with an attention that reads a
// segment once for all of them and the wide step's one-product classifier.  Also the two hooks that run the row launch and
// the GEMM on their own.
#include <algorithm>
#include <cstring>
#include <vector>

#include "batch_host.h"
#include "kind_rows.h"
#include "kv8.h"
#include "kv8_layout.h"
#include "wide_decode.h"

using namespace l2z;

namespace {

// The rows of a pass and where its launches put them: m rows; the residual rows x, dim apart; a layer's attention output
// att and the gated rows h at their pitches; the quantized rows xq and their scales xs (group size gs) that every product
// reads; st: the pass's stream; by_rows: the pass's products take the form its row count picks (q8_gemm_form: the wide
// step), else launch_q8_gemm whatever m is
struct Q8Rows {
    int m;
    float *x, *att, *h;
    int ld_att, ld_h;
    int8_t *xq;
    float *xs;
    int gs;
    hipStream_t st;
    bool by_rows;
};

// THE form choice of a product of m rows where it is made by the shape: the bits are the same either
// way, so the thresholds are measurement's to move.  From 17 rows on the register-blocked form, where its blocks of 32 weight
// rows are at least one a CU: W1 | W3 and the classifier of the 7B shape (688 and 1000 blocks, 1.33 - 1.50 x q8_gemm_kernel at
// 32 - 128 rows), not its 4096-row products (128 blocks on 256 CUs: 0.75 - 0.85 x; profiles/q8_wide_bench.md).  The
// threshold rests on those two points: at exactly one block a CU (d = 8192 on 256 CUs) nothing has been measured
hipError_t q8_gemm_form(const Q8GemmArgs &a, int epi, hipStream_t st)
{
    const bool wide = a.m > kQ8GemmTile && (a.d + 31) / 32 >= g_cus;
    return wide ? launch_q8_gemm_wide(a, epi, st) : launch_q8_gemm(a, epi, st);
}

// rows of `x`, ldx apart (after the rmsnorm with rms_w, if any), quantized over k -> r.xq, r.xs
int q8_quantize(const Q8Rows &r, const float *x, int ldx, int k, const float *rms_w)
{
    L2Z_HIP(launch_q8_quantize_rows(x, ldx, r.m, k, rms_w, r.gs, r.xq, r.xs, r.st));
    return L2Z_OK;
}

// ... and their product with layer l's [d, k] matrix of m -> out, through the epilogue epi (the residual is out itself)
int q8_product(const Q8Rows &r, const l2z_weights::Q8Mat &m, int l, int d, int k, float *out, int ldo, int epi)
{
    const size_t at = (size_t)l * (size_t)d * (size_t)k;
    Q8GemmArgs a = {};
    a.xq = r.xq; a.xs = r.xs; a.wq = m.q + at; a.ws = m.s + at / (size_t)r.gs;
    a.out = out; a.ldo = ldo; a.res = out; a.ldres = ldo;
    a.m = r.m; a.n = k; a.d = d; a.gs = r.gs;
    L2Z_HIP(r.by_rows ? q8_gemm_form(a, epi, r.st) : launch_q8_gemm(a, epi, r.st));
    return L2Z_OK;
}

// The layers of a pass over r.x.  qkv_attention(l, layer_off) finds layer l's quantized rows in r.xq / r.xs, writes the
// rows' k | v into the caches, layer_off floats in, and leaves the attention output in r.att.
int q8_layers(const Q8Rows &r, const l2z_config &c, const l2z_weights *w, FnRef<int(int, size_t)> qkv_attention)
{
    const int dim = c.dim, hid = c.hidden_dim, kvd = dim / c.n_heads * c.n_kv_heads;
    for (int l = 0; l < c.n_layers; l++) {
        L2Z_TRY(q8_quantize(r, r.x, dim, dim, w->rms_att + (size_t)l * dim));       // :305
        L2Z_TRY(qkv_attention(l, (size_t)l * c.seq_len * kvd));                     // :308-389
        L2Z_TRY(q8_quantize(r, r.att, r.ld_att, dim, nullptr));
        L2Z_TRY(q8_product(r, w->q_wo, l, dim, dim, r.x, dim, EPI_RESID));          // :392-395
        L2Z_TRY(q8_quantize(r, r.x, dim, dim, w->rms_ffn + (size_t)l * dim));       // :398
        L2Z_TRY(q8_product(r, w->q_w13, l, 2 * hid, dim, r.h, r.ld_h, EPI_SWIGLU));  // :405-416
        L2Z_TRY(q8_quantize(r, r.h, r.ld_h, hid, nullptr));
        L2Z_TRY(q8_product(r, w->q_w2, l, dim, hid, r.x, dim, EPI_RESID));          // :419-422
    }
    return L2Z_OK;
}

// The pass's scratch, one allocation owned by the runstate (l2z_runstate::q8pf, freed with it), carved for chunks of up to
// `cap` rows: the residual rows, q | k | v, the attention output and the gated rows in f32; the quantized rows and their
// scales at the widest K; the tokens and the one-sequence table of the scatter.  Behind them, in a runstate with int8 KV
// rows alone (l2z_prefill_kv8; the f32 runstate's carving is what it was): the slots and the slices' tables of the prompt
// attention's row form (kv8.h Kv8Prompt) and the wide step's partials
struct Q8Pf {
    float *x, *q, *k, *v, *att, *h, *xs;
    int8_t *xq;
    int *tokens, *row_seq, *row_pos;
    RaggedSeq *seq;
    void *kv8_tab;
    float *kv8_part;
    size_t bytes;
};

Q8Pf q8pf_carve(const l2z_runstate *s, int gs, size_t cap)
{
    const l2z_config &c = s->cfg;
    const size_t dim = c.dim, hid = c.hidden_dim, kvd = s->sh.kvd_loc, widest = std::max(dim, hid);
    uint8_t *base = (uint8_t *)s->q8pf.get();
    size_t off = 0;
    const auto take = [&](size_t bytes) {
        uint8_t *p = base + off;
        off = (off + bytes + 255) & ~(size_t)255;
        return p;
    };
    Q8Pf b = {};
    b.x = (float *)take(cap * dim * 4);
    b.q = (float *)take(cap * dim * 4);
    b.k = (float *)take(cap * kvd * 4);
    b.v = (float *)take(cap * kvd * 4);
    b.att = (float *)take(cap * dim * 4);
    b.h = (float *)take(cap * hid * 4);
    b.xq = (int8_t *)take(cap * widest);
    b.xs = (float *)take(cap * (widest / (size_t)gs) * 4);
    b.tokens = (int *)take(cap * 4);
    b.row_seq = (int *)take(cap * 4);
    b.row_pos = (int *)take(cap * 4);
    b.seq = (RaggedSeq *)take(sizeof(RaggedSeq));
    if (s->is_kv8()) {
        b.kv8_tab = take(kv8_prompt_table_bytes((int)cap, true));
        b.kv8_part = (float *)take(wide_part_floats(c.n_heads, verify_segments(c.seq_len), s->sh.hs) * 4);
    }
    b.bytes = off;
    return b;
}

int q8pf_alloc(l2z_runstate *s, int gs, int need)
{
    const size_t cap = (size_t)round_cap(need, 512);   // as prefill_alloc (a multiple of the GEMM's tile)
    return grow("l2z_prefill_q8 scratch", &s->q8pf_cap, need, 512, &s->q8pf_gs, gs, [&] { return drain_stream(s); },
                {{s->q8pf, q8pf_carve(s, gs, cap).bytes}});
}

// A chunk's launch between its q | k | v products and its attention -- q [P, dim] rotated in place, the chunk's k / v rows
// into the sequence's cache through the one-sequence table rg -- and its causal attention into b.att, as the pass's owner
// brings them: the f32 caches' (l2z_prefill_q8) or the int8 rows' (l2z_prefill_kv8), the way wide_step_q8 takes rg.scatter /
// rg.attention
using Q8Scatter = FnRef<hipError_t(const RaggedChunk &rg, int P, size_t layer_off)>;
using Q8Attention = FnRef<hipError_t(int pos0, int P, size_t layer_off)>;

// one chunk: rows pos0 .. pos0 + P - 1 through every layer; the residual rows are left in b.x
int q8_chunk(l2z_runstate *s, const l2z_weights *w, const Q8Pf &b, const int32_t *tokens, int P, int pos0, Q8Scatter scatter,
             Q8Attention attention)
{
    const l2z_config &c = s->cfg;
    hipStream_t st = s->stream;
    const int dim = c.dim, kvd = s->sh.kvd_loc;
    L2Z_HIP(hipMemcpyAsync(b.tokens, tokens, (size_t)P * 4, hipMemcpyHostToDevice, st));
    L2Z_HIP(launch_q8_embed_rows(w->q8_emb(), b.tokens, dim, P, b.x, pos0, b.row_seq, b.row_pos, st));
    RaggedChunk rg = {};
    rg.seq = b.seq; rg.row_seq = b.row_seq; rg.row_pos = b.row_pos;
    rg.n_seq = 1; rg.seq_max = 1; rg.k = b.k; rg.v = b.v;
    const Q8Rows r = {P, b.x, b.att, b.h, dim, c.hidden_dim, b.xq, b.xs, w->q8_gs, st, false};   // (every pitch tight)
    return q8_layers(r, c, w, [&](int l, size_t layer_off) -> int {
        L2Z_TRY(q8_product(r, w->q_wq, l, dim, dim, b.q, dim, EPI_STORE));        // :308-320
        L2Z_TRY(q8_product(r, w->q_wk, l, kvd, dim, b.k, kvd, EPI_STORE));
        L2Z_TRY(q8_product(r, w->q_wv, l, kvd, dim, b.v, kvd, EPI_STORE));
        L2Z_HIP(scatter(rg, P, layer_off));        // :336-358
        L2Z_HIP(attention(pos0, P, layer_off));    // :361-389
        return L2Z_OK;
    });
}

// the decode's final rmsnorm + classifier launch on s->x, argmax candidates included (forward.cpp)
int q8_classifier(l2z_runstate *s, const l2z_weights *w)
{
    const l2z_config &c = s->cfg;
    Q8MatvecArgs a = {};
    a.b.out0 = s->logits; a.b.rows0 = c.vocab_size; a.b.n = c.dim; a.b.rms_w = w->rms_final; a.b.x = s->x;
    a.b.part_val = s->d_part_val; a.b.part_idx = s->d_part_idx; a.b.row_offset = 0;
    a.gs = w->q8_gs;
    attach_rows(a, kind_rows(w, s->sh, KIND_CLS, 0));
    int grid = 0;
    L2Z_HIP(launch_q8_matvec(a, EPI_ARGMAX, s->max_blocks, g_cus, s->stream, &grid));
    s->n_part = grid;
    return L2Z_OK;
}

// l2z_prefill_q8 (kv8 false: an f32 runstate) and l2z_prefill_kv8 (true: one with int8 KV rows): one front,
// one chunk loop; they differ in the kind of runstate they take and in the scatter and the attention they hand q8_chunk
int prefill_q8_pass(const char *fn, bool kv8, const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
                    const l2z_weights *w)
{
    // ---- checks: a refusal enqueues nothing and changes no state ----
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && config != nullptr && s != nullptr && w != nullptr, L2Z_ERR_INVALID, "%s: null argument", fn);
    L2Z_CHECK(n_tokens >= 1, L2Z_ERR_INVALID, "%s: n_tokens = %d (at least 1)", fn, n_tokens);
    L2Z_CHECK(w->is_q8(), L2Z_ERR_INVALID,
              "%s: takes int8 group-quantized weights (l2z_weights_init_q8); f32 and packed weights go to l2z_prefill", fn);
    L2Z_CHECK(!kv8 || s->is_kv8(), L2Z_ERR_INVALID,
              "l2z_prefill_kv8: takes a runstate with int8 KV rows (l2z_runstate_init_kv8); every other one goes to l2z_prefill_q8");
    L2Z_TRY(check_pair(config, s, w, false, true, kv8));   // (a sharded or paged runstate, another config; kv8 false: int8 KV rows)
    const int hs = s->sh.hs;
    L2Z_CHECK(hs % 4 == 0 && hs <= 256 && s->sh.kvd_loc % 4 == 0, L2Z_ERR_INVALID,
              "%s: needs a head_size that is a multiple of 4, at most 256", fn);
    L2Z_TRY(check_positions(fn, "", "positions", pos0, n_tokens, config->seq_len));
    L2Z_TRY(check_tokens(fn, "", tokens, n_tokens, config->vocab_size));
    L2Z_HIP(hipSetDevice(s->device));
    int longest = 0;   // the plan's longest chunk sizes the scratch before anything is enqueued
    for (int done = 0; done < n_tokens;) {
        const int P = prefill_next_chunk_of(*config, n_tokens - done);
        longest = std::max(longest, P);
        done += P;
    }
    L2Z_TRY(q8pf_alloc(s, w->q8_gs, longest));
    const Q8Pf b = q8pf_carve(s, w->q8_gs, (size_t)s->q8pf_cap);

    // ---- the pass ----
    const l2z_config &c = s->cfg;
    hipStream_t st = s->stream;
    const int dim = c.dim, kvd = s->sh.kvd_loc, kv_mul = c.n_heads / c.n_kv_heads;
    const size_t kvh_stride = (size_t)c.seq_len * hs;
    RaggedSeq seq = {};
    seq.kc = s->key_cache; seq.vc = s->value_cache;
    L2Z_HIP(hipMemcpyAsync(b.seq, &seq, sizeof seq, hipMemcpyHostToDevice, st));
    // the f32 caches: the f32 pass's RoPE + cache scatter and its prompt attention
    const auto scatter32 = [&](const RaggedChunk &rg, int P, size_t layer_off) {
        return launch_ragged_rope_scatter(b.q, dim, rg, P, dim, kvd, hs, s->rope, layer_off, kvh_stride, st);
    };
    const auto attention32 = [&](int p0, int P, size_t layer_off) {
        return launch_prefill_attention(b.q, dim, s->key_cache + layer_off, s->value_cache + layer_off, b.att, dim, p0, P, c.n_heads, hs,
                                        hs, kvh_stride, kv_mul, c.seq_len, st, c.n_heads);
    };
    // int8 rows: the format's scatter FIRST, then the attention over the int8 arrays alone, the chunk's own rows included
    Kv8Prompt pr = {};
    pr.seq = {s->k8, s->v8, s->ks8, s->vs8};
    if (kv8) {
        pr.slots = (const Kv8Seq *)b.kv8_tab;
        pr.tab = (const WideTable *)(pr.slots + kWideMax);
        pr.part = b.kv8_part;
        pr.seg_cap = verify_segments(c.seq_len);
    }
    const auto scatter8 = [&](const RaggedChunk &rg, int P, size_t layer_off) {
        return launch_kv8_rope_scatter(b.q, dim, rg, pr.slots, P, dim, kvd, hs, c.seq_len, s->rope, layer_off, kvh_stride, st);
    };
    const auto attention8 = [&](int p0, int P, size_t layer_off) {
        return launch_kv8_prefill_attention(b.q, dim, pr, b.att, dim, p0, P, c.n_heads, hs, kv_mul, c.seq_len, layer_off, kvh_stride, st);
    };
    std::vector<uint8_t> tab;   // the chunk's slots and row tables on the host, alive until the chunk's synchronize
    for (int done = 0; done < n_tokens;) {
        const int P = prefill_next_chunk_of(*config, n_tokens - done);
        if (kv8) {   // one copy before the layer loop
            const bool with_rows = !kv8_prefill_flash_shape(hs, P);
            tab.resize(kv8_prompt_table_bytes(P, with_rows));
            kv8_prompt_tables(tab.data(), pr.seq, pos0 + done, P, with_rows);
            L2Z_HIP(hipMemcpyAsync(b.kv8_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
            L2Z_TRY(q8_chunk(s, w, b, tokens + done, P, pos0 + done, scatter8, attention8));
        } else {
            L2Z_TRY(q8_chunk(s, w, b, tokens + done, P, pos0 + done, scatter32, attention32));
        }
        if (done + P == n_tokens)   // the last position's residual row is RunState.x
            L2Z_HIP(hipMemcpyAsync(s->x, b.x + (size_t)(P - 1) * config->dim, (size_t)config->dim * 4, hipMemcpyDeviceToDevice, st));
        L2Z_HIP(hipStreamSynchronize(st));   // the caller's tokens may now be reused
        done += P;
    }
    const int last_pos = pos0 + n_tokens - 1;
    L2Z_HIP(hipMemcpyAsync(s->d_pos, &last_pos, sizeof(int), hipMemcpyHostToDevice, st));
    L2Z_HIP(hipMemcpyAsync(s->d_token, &tokens[n_tokens - 1], sizeof(int), hipMemcpyHostToDevice, st));
    L2Z_TRY(q8_classifier(s, w));
    s->logits_partial = false;
    L2Z_HIP(hipStreamSynchronize(st));
    s->host_pos = pos0 + n_tokens;
    return L2Z_OK;
}

}  // namespace

extern "C" int l2z_prefill_q8(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
                              const l2z_weights *w)
{
    return prefill_q8_pass("l2z_prefill_q8", false, tokens, n_tokens, pos0, config, s, w);
}

// PREVIEW (include/llama2_hip_test.h): l2z_prefill_q8's contract on a runstate with int8 KV rows
extern "C" int l2z_prefill_kv8(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
                               const l2z_weights *w)
{
    return prefill_q8_pass("l2z_prefill_kv8", true, tokens, n_tokens, pos0, config, s, w);
}

// The step on int8 group-quantized weights.  Per layer q | k | v in one launch (RoPE and the cache rows in
// its epilogue) and the caller's attention; then the classifier through the table.  Every product is the one-tile form of
// q8_gemm_device.h: a row's bits do not depend on n, on the other rows, or on its place in the batch.
int l2z::batch_step_q8(int n, const l2z_config &c, l2z_runstate *s0, const l2z_weights *w, BatchScratch *b, LayerAttention attention)
{
    hipStream_t st = s0->stream;
    const int dim = c.dim, hs = dim / c.n_heads, kvd = hs * c.n_kv_heads, gs = w->q8_gs;
    const BatchTable *tab = b->d_tab;
    const Q8Rows r = {n, b->x, b->att, b->h1, b->ld_att, b->ld_h1, b->q8_xq, b->q8_xs, gs, st, false};
    L2Z_HIP(launch_q8_embed_rows(w->q8_emb(), tab->tokens, dim, n, b->x, 0, nullptr, nullptr, st));  // :295
    L2Z_TRY(q8_layers(r, c, w, [&](int l, size_t layer_off) -> int {
        // q | k | v (:308-358): RoPE at each row's own position, k | v into each row's own caches
        const size_t at_q = (size_t)l * dim * dim, at_kv = (size_t)l * kvd * dim;
        Q8BatchQkvArgs a = {};
        a.xq = r.xq; a.xs = r.xs;
        a.wq_q = w->q_wq.q + at_q; a.ws_q = w->q_wq.s + at_q / (size_t)gs;
        a.wq_k = w->q_wk.q + at_kv; a.ws_k = w->q_wk.s + at_kv / (size_t)gs;
        a.wq_v = w->q_wv.q + at_kv; a.ws_v = w->q_wv.s + at_kv / (size_t)gs;
        a.q = b->q; a.ldq = dim; a.tab = tab; a.rope = s0->rope;
        a.layer_off = layer_off; a.kv_head_stride = (size_t)c.seq_len * hs;
        a.m = n; a.n = dim; a.dim = dim; a.kvd = kvd; a.hs = hs; a.gs = gs;
        L2Z_HIP(launch_q8_batch_qkv(a, st));
        return attention(layer_off);  // :361-389
    }));
    L2Z_TRY(q8_quantize(r, b->x, dim, dim, w->rms_final));  // :426
    Q8BatchClsArgs a = {};   // :429: each row's logits straight into its runstate
    a.xq = r.xq; a.xs = r.xs; a.wq = w->q_cls.q; a.ws = w->q_cls.s; a.tab = tab;
    a.m = n; a.n = dim; a.vocab = c.vocab_size; a.gs = gs;
    L2Z_HIP(launch_q8_batch_cls(a, st));
    return L2Z_OK;
}

// The wide step on int8 group-quantized weights (l2z_transformer_wide_q8): n <= kWideMax rows on s0's prompt
// scratch (wide_begin has sized it), the rows' tokens, positions and caches in the table rg reads.  Per layer q, k and v are
// three products into scratch, then the ragged pass's RoPE + cache scatter over the table -- or the table owner's launch in its
// place (rg.scatter: int8 KV rows) -- and the table owner's attention
// (no bf16 planes: the Wo product reads quantized rows); after the layers the classifier as ONE product into logits
// [n, ld_logits].  Every product takes the form its row count picks.
int l2z::wide_step_q8(int n, l2z_runstate *s0, const l2z_weights *w, const RaggedChunk &rg, const int *tokens, int8_t *xq, float *xs,
                      float *logits, int ld_logits)
{
    const l2z_config &c = s0->cfg;
    hipStream_t st = s0->stream;
    const int dim = c.dim, hs = s0->sh.hs, kvd = s0->sh.kvd_loc;
    const size_t kvh_stride = (size_t)c.seq_len * hs;
    const Q8Rows r = {n, s0->pf_x, s0->pf_att, s0->pf_h1, s0->pf_ld_att, s0->pf_ld_h1, xq, xs, w->q8_gs, st, true};
    L2Z_HIP(launch_q8_embed_rows(w->q8_emb(), tokens, dim, n, r.x, 0, nullptr, nullptr, st));   // :295
    L2Z_TRY(q8_layers(r, c, w, [&](int l, size_t layer_off) -> int {
        L2Z_TRY(q8_product(r, w->q_wq, l, dim, dim, s0->pf_q, dim, EPI_STORE));     // :308-320
        L2Z_TRY(q8_product(r, w->q_wk, l, kvd, dim, rg.k, kvd, EPI_STORE));
        L2Z_TRY(q8_product(r, w->q_wv, l, kvd, dim, rg.v, kvd, EPI_STORE));
        if (rg.scatter != nullptr) L2Z_HIP((*rg.scatter)(s0->pf_q, dim, n, layer_off, kvh_stride, st));   // (int8 KV rows, kv8.h)
        else L2Z_HIP(launch_ragged_rope_scatter(s0->pf_q, dim, rg, n, dim, kvd, hs, s0->rope, layer_off, kvh_stride, st));   // :336-358
        const RaggedLayer L = {s0->pf_q, dim, s0->pf_att, s0->pf_ld_att, n, c.n_heads, hs, c.n_heads / c.n_kv_heads, c.seq_len,
                               layer_off, kvh_stride, st, nullptr, 0};
        L2Z_HIP((*rg.attention)(L, nullptr));   // :361-389
        return L2Z_OK;
    }));
    L2Z_TRY(q8_quantize(r, r.x, dim, dim, w->rms_final));   // :426
    return q8_product(r, w->q_cls, 0, c.vocab_size, dim, logits, ld_logits, EPI_STORE);   // :429
}

// The verify pass over int8 KV rows (l2z_verify_kv8, verify_host.cpp): n <= kBatchMax rows of ONE sequence at
// positions pos0 .., on the prompt pass's scratch (verify_kv8_scratch has sized it).  It is the chunk l2z_prefill_kv8 runs
// for those rows -- the same products, launch_kv8_rope_scatter over the one-sequence table -- with two differences: the
// layers' attention is launch_kv8_verify_attention, which reads a segment's bytes once for all rows, and the classifier
// runs as ONE product over all rows into logits [n, ld_logits], as wide_step_q8 ends.  Nothing comes up from the host here:
// tokens and seq8 (slot 0 = the sequence's arrays) stand on the device behind the caller's table copy, and the rows'
// positions are written by the embed launch -- into the pos[] of the WideTable wide_combine reads and the scatter's row_pos
// at once.
int l2z::verify_kv8_scratch(l2z_runstate *s, const l2z_weights *w) { return q8pf_alloc(s, w->q8_gs, kBatchMax); }

int l2z::verify_kv8_pass(int n, int pos0, l2z_runstate *s, const l2z_weights *w, const int *tokens, const Kv8Seq *seq8, float *logits,
                         int ld_logits)
{
    const l2z_config &c = s->cfg;
    hipStream_t st = s->stream;
    const int dim = c.dim, hs = s->sh.hs, kvd = s->sh.kvd_loc;
    const size_t kvh_stride = (size_t)c.seq_len * hs;
    const Q8Pf b = q8pf_carve(s, w->q8_gs, (size_t)s->q8pf_cap);
    const WideTable *tab = (const WideTable *)((const Kv8Seq *)b.kv8_tab + kWideMax);   // (kv8.h Kv8Prompt: behind the slots)
    int *row_pos = const_cast<int32_t *>(tab->pos);
    L2Z_HIP(launch_q8_embed_rows(w->q8_emb(), tokens, dim, n, b.x, pos0, b.row_seq, row_pos, st));   // :295
    RaggedChunk rg = {};
    rg.seq = b.seq; rg.row_seq = b.row_seq; rg.row_pos = row_pos;
    rg.n_seq = 1; rg.seq_max = 1; rg.k = b.k; rg.v = b.v;
    const WideAttn wa = {tab, b.kv8_part, verify_segments(c.seq_len), (pos0 + n - 1) / kVerifySeg + 1, 0, 1, 0};
    const Q8Rows r = {n, b.x, b.att, b.h, dim, c.hidden_dim, b.xq, b.xs, w->q8_gs, st, false};   // (every pitch tight)
    L2Z_TRY(q8_layers(r, c, w, [&](int l, size_t layer_off) -> int {
        L2Z_TRY(q8_product(r, w->q_wq, l, dim, dim, b.q, dim, EPI_STORE));        // :308-320
        L2Z_TRY(q8_product(r, w->q_wk, l, kvd, dim, b.k, kvd, EPI_STORE));
        L2Z_TRY(q8_product(r, w->q_wv, l, kvd, dim, b.v, kvd, EPI_STORE));
        L2Z_HIP(launch_kv8_rope_scatter(b.q, dim, rg, seq8, n, dim, kvd, hs, c.seq_len, s->rope, layer_off, kvh_stride, st));   // :336-358
        const RaggedLayer L = {b.q, dim, b.att, dim, n, c.n_heads, hs, c.n_heads / c.n_kv_heads, c.seq_len, layer_off, kvh_stride, st, nullptr, 0};
        L2Z_HIP(launch_kv8_verify_attention(L, wa, seq8, 0, pos0));                 // :361-389
        return L2Z_OK;
    }));
    L2Z_TRY(q8_quantize(r, r.x, dim, dim, w->rms_final));   // :426
    return q8_product(r, w->q_cls, 0, c.vocab_size, dim, logits, ld_logits, EPI_STORE);   // :429
}

// ---------------------------------------------------------------------------
// The pass's two launches on their own (host pointers, synchronous)
extern "C" int l2z_q8_quantize_rows(const float *x, int m, size_t n, const float *rms_w, int gs, int8_t *out_q, float *out_s)
{
    L2Z_CHECK(x && out_q && out_s && m > 0 && m <= (1 << 20) && n > 0 && n < (1u << 24), L2Z_ERR_INVALID, "l2z_q8_quantize_rows: bad arguments");
    L2Z_CHECK((gs == 32 || gs == 64) && n % (size_t)gs == 0, L2Z_ERR_INVALID,
              "l2z_q8_quantize_rows: group size %d (32 or 64, dividing n = %zu)", gs, n);
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const size_t mp = (size_t)q8_gemm_rows_padded(m), ng = n / (size_t)gs;
    HookBuf<void> dx, dw, dq, ds;
    L2Z_TRY(dx.alloc((size_t)m * n * 4)); L2Z_TRY(dw.alloc(n * 4)); L2Z_TRY(dq.alloc(mp * n)); L2Z_TRY(ds.alloc(mp * ng * 4));
    L2Z_HIP(hipMemcpy(dx.p.get(), x, (size_t)m * n * 4, hipMemcpyHostToDevice));
    if (rms_w) L2Z_HIP(hipMemcpy(dw.p.get(), rms_w, n * 4, hipMemcpyHostToDevice));
    L2Z_HIP(launch_q8_quantize_rows((const float *)dx.p.get(), (int)n, m, (int)n, rms_w ? (const float *)dw.p.get() : nullptr, gs, (int8_t *)dq.p.get(),
                                    (float *)ds.p.get(), nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    L2Z_HIP(hipMemcpy(out_q, dq.p.get(), (size_t)m * n, hipMemcpyDeviceToHost));
    L2Z_HIP(hipMemcpy(out_s, ds.p.get(), (size_t)m * ng * 4, hipMemcpyDeviceToHost));
    return L2Z_OK;
}

namespace {
// l2z_q8_gemm (wide false) and l2z_q8_gemm_wide (true), both with the store epilogue, and l2z_q8_gemm_epi: one body, the
// launcher and the epilogue apart.  EPI_RESID: out holds the residual on entry and is both on the device, as the pass's Wo and
// W2 launches; EPI_SWIGLU: out is [m, d / 2]
int q8_gemm_hook(const char *fn, bool wide, int epi, float *out, const int8_t *xq, const float *xs, int m, const int8_t *wq, const float *ws,
                 size_t n, size_t d, int gs)
{
    L2Z_CHECK(out && xq && xs && wq && ws && m > 0 && m <= (1 << 20) && n > 0 && d > 0 && n < (1u << 24) && d < (1u << 24),
              L2Z_ERR_INVALID, "%s: bad arguments", fn);
    L2Z_CHECK(epi == EPI_STORE || epi == EPI_RESID || epi == EPI_SWIGLU, L2Z_ERR_INVALID, "%s: epi = %d (0 store, 2 residual, 3 SwiGLU)", fn, epi);
    L2Z_CHECK(!wide || (m >= 17 && m <= kWideMax), L2Z_ERR_INVALID, "%s: m = %d outside [17, %d] (fewer rows go to l2z_q8_gemm)", fn, m, kWideMax);
    L2Z_CHECK((gs == 32 || gs == 64) && n % (size_t)gs == 0, L2Z_ERR_INVALID,
              "%s: group size %d (32 or 64, dividing n = %zu)", fn, gs, n);
    L2Z_CHECK(d % 4 == 0, L2Z_ERR_INVALID, "%s: d = %zu (a multiple of 4: a lane stores four features)", fn, d);
    L2Z_CHECK(epi != EPI_SWIGLU || d % 8 == 0, L2Z_ERR_INVALID, "%s: d = %zu (SwiGLU: a multiple of 8, the gated rows' pitch one of 4)", fn, d);
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const size_t mp = (size_t)q8_gemm_rows_padded(m), ng = n / (size_t)gs;
    HookBuf<void> dxq, dxs, dwq, dws, dout;
    L2Z_TRY(dxq.alloc(mp * n)); L2Z_TRY(dxs.alloc(mp * ng * 4)); L2Z_TRY(dwq.alloc(d * n)); L2Z_TRY(dws.alloc(d * ng * 4));
    const size_t out_bytes = (size_t)m * (epi == EPI_SWIGLU ? d / 2 : d) * 4;
    L2Z_TRY(dout.alloc((size_t)m * d * 4));
    if (epi == EPI_RESID) L2Z_HIP(hipMemcpy(dout.p.get(), out, out_bytes, hipMemcpyHostToDevice));
    // the rows stand padded to whole tiles, the pad rows zero, as the row launch leaves them
    L2Z_HIP(hipMemset(dxq.p.get(), 0, mp * n));
    L2Z_HIP(hipMemset(dxs.p.get(), 0, mp * ng * 4));
    L2Z_HIP(hipMemcpy(dxq.p.get(), xq, (size_t)m * n, hipMemcpyHostToDevice));
    L2Z_HIP(hipMemcpy(dxs.p.get(), xs, (size_t)m * ng * 4, hipMemcpyHostToDevice));
    L2Z_HIP(hipMemcpy(dwq.p.get(), wq, d * n, hipMemcpyHostToDevice));
    L2Z_HIP(hipMemcpy(dws.p.get(), ws, d * ng * 4, hipMemcpyHostToDevice));
    Q8GemmArgs a = {};
    a.xq = (const int8_t *)dxq.p.get(); a.xs = (const float *)dxs.p.get(); a.wq = (const int8_t *)dwq.p.get(); a.ws = (const float *)dws.p.get();
    a.out = (float *)dout.p.get(); a.ldo = (int)(epi == EPI_SWIGLU ? d / 2 : d);
    a.res = a.out; a.ldres = a.ldo;
    a.m = m; a.n = (int)n; a.d = (int)d; a.gs = gs;
    L2Z_HIP(wide ? launch_q8_gemm_wide(a, epi, nullptr) : launch_q8_gemm(a, epi, nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    L2Z_HIP(hipMemcpy(out, dout.p.get(), out_bytes, hipMemcpyDeviceToHost));
    return L2Z_OK;
}
}  // namespace

extern "C" int l2z_q8_gemm(float *out, const int8_t *xq, const float *xs, int m, const int8_t *wq, const float *ws, size_t n,
                           size_t d, int gs)
{
    return q8_gemm_hook("l2z_q8_gemm", false, EPI_STORE, out, xq, xs, m, wq, ws, n, d, gs);
}

// PREVIEW (include/llama2_hip_test.h): the register-blocked form on its own, 17 <= m <= L2Z_WIDE_MAX
extern "C" int l2z_q8_gemm_wide(float *out, const int8_t *xq, const float *xs, int m, const int8_t *wq, const float *ws, size_t n,
                                size_t d, int gs)
{
    return q8_gemm_hook("l2z_q8_gemm_wide", true, EPI_STORE, out, xq, xs, m, wq, ws, n, d, gs);
}

// PREVIEW (include/llama2_hip_test.h): ONE launch of either form with any of the three epilogues, as the passes issue it
extern "C" int l2z_q8_gemm_epi(int epi, int wide, float *out, const int8_t *xq, const float *xs, int m, const int8_t *wq,
                               const float *ws, size_t n, size_t d, int gs)
{
    return q8_gemm_hook("l2z_q8_gemm_epi", wide != 0, epi, out, xq, xs, m, wq, ws, n, d, gs);
}
