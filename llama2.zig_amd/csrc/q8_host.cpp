// q8_host.cpp -- host side of the multi-row passes on int8 group-quantized weights: the prompt pass l2z_prefill_q8
// (include/llama2_hip_test.h) and the batched step behind l2z_transformer_batch_q8 and l2z_verify_q8
// (batch_step_q8).  Both go through ONE layer walk (q8_layers), apart from the f32 walks
// of prefill_host.cpp and batch_step: per layer four row launches (q8_rows.hip: the group quantization of the pass's rows,
// after the rmsnorm where the decode's launch has one) and, behind the attention, three GEMM launches on the int8 matrix
// cores (q8_gemm.hip: Wo and W2 with the residual, W1 | W3 with SwiGLU).  How q | k | v, the cache rows and the attention
// output come about is the caller's: the prompt pass runs three more GEMMs into scratch, the f32 pass's RoPE + cache
// scatter over a one-sequence table and its prompt attention, and sends the last row through the decode's own classifier
// launch, so the runstate is left as after a decode step; the step runs q | k | v as one launch (q8_batch.hip), its
// caller's attention and the classifier through the table.  Also the two hooks that run the row launch and the GEMM on
// their own.
#include <algorithm>
#include <cstring>

#include "batch_host.h"
#include "kind_rows.h"

using namespace l2z;

namespace {

// The rows of a pass and where its launches put them: m rows; the residual rows x, dim apart; a layer's attention output
// att and the gated rows h at their pitches; the quantized rows xq and their scales xs (group size gs) that every product
// reads; st: the pass's stream
struct Q8Rows {
    int m;
    float *x, *att, *h;
    int ld_att, ld_h;
    int8_t *xq;
    float *xs;
    int gs;
    hipStream_t st;
};

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
    L2Z_HIP(launch_q8_gemm(a, epi, r.st));
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
// scales at the widest K; the tokens and the one-sequence table of the scatter
struct Q8Pf {
    float *x, *q, *k, *v, *att, *h, *xs;
    int8_t *xq;
    int *tokens, *row_seq, *row_pos;
    RaggedSeq *seq;
    size_t bytes;
};

Q8Pf q8pf_carve(const l2z_runstate *s, int gs, size_t cap)
{
    const l2z_config &c = s->cfg;
    const size_t dim = c.dim, hid = c.hidden_dim, kvd = s->sh.kvd_loc, widest = std::max(dim, hid);
    uint8_t *base = (uint8_t *)s->q8pf;
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
    b.bytes = off;
    return b;
}

int q8pf_alloc(l2z_runstate *s, int gs, int need)
{
    if (s->q8pf != nullptr && s->q8pf_cap >= need && s->q8pf_gs == gs) return L2Z_OK;
    const size_t cap = (size_t)(need + 511) / 512 * 512;   // as prefill_alloc (a multiple of the GEMM's tile)
    L2Z_HIP(hipStreamSynchronize(s->stream));
    if (s->q8pf) { (void)hipFree(s->q8pf); s->q8pf = nullptr; }
    s->q8pf_cap = 0;
    const size_t bytes = q8pf_carve(s, gs, cap).bytes;
    L2Z_TRY(alloc_all("l2z_prefill_q8 scratch", {{&s->q8pf, bytes}}));
    s->q8pf_cap = (int)cap;
    s->q8pf_gs = gs;
    return L2Z_OK;
}

// one chunk: rows pos0 .. pos0 + P - 1 through every layer; the residual rows are left in b.x
int q8_chunk(l2z_runstate *s, const l2z_weights *w, const Q8Pf &b, const int32_t *tokens, int P, int pos0)
{
    const l2z_config &c = s->cfg;
    hipStream_t st = s->stream;
    const int dim = c.dim, kvd = s->sh.kvd_loc, hs = s->sh.hs;
    const size_t kvh_stride = (size_t)c.seq_len * hs;
    L2Z_HIP(hipMemcpyAsync(b.tokens, tokens, (size_t)P * 4, hipMemcpyHostToDevice, st));
    L2Z_HIP(launch_q8_embed_rows(w->q8_emb(), b.tokens, dim, P, b.x, pos0, b.row_seq, b.row_pos, st));
    RaggedChunk rg = {};
    rg.seq = b.seq; rg.row_seq = b.row_seq; rg.row_pos = b.row_pos;
    rg.n_seq = 1; rg.seq_max = 1; rg.k = b.k; rg.v = b.v;
    const Q8Rows r = {P, b.x, b.att, b.h, dim, c.hidden_dim, b.xq, b.xs, w->q8_gs, st};   // (every pitch tight)
    return q8_layers(r, c, w, [&](int l, size_t layer_off) -> int {
        L2Z_TRY(q8_product(r, w->q_wq, l, dim, dim, b.q, dim, EPI_STORE));        // :308-320
        L2Z_TRY(q8_product(r, w->q_wk, l, kvd, dim, b.k, kvd, EPI_STORE));
        L2Z_TRY(q8_product(r, w->q_wv, l, kvd, dim, b.v, kvd, EPI_STORE));
        L2Z_HIP(launch_ragged_rope_scatter(b.q, dim, rg, P, dim, kvd, hs, s->rope, layer_off, kvh_stride, st));   // :336-358
        L2Z_HIP(launch_prefill_attention(b.q, dim, s->key_cache + layer_off, s->value_cache + layer_off, b.att, dim, pos0, P,
                                         c.n_heads, hs, hs, kvh_stride, c.n_heads / c.n_kv_heads, c.seq_len, st, c.n_heads));   // :361-389
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

}  // namespace

extern "C" int l2z_prefill_q8(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
                              const l2z_weights *w)
{
    // ---- checks: a refusal enqueues nothing and changes no state ----
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && config != nullptr && s != nullptr && w != nullptr, L2Z_ERR_INVALID, "l2z_prefill_q8: null argument");
    L2Z_CHECK(n_tokens >= 1, L2Z_ERR_INVALID, "l2z_prefill_q8: n_tokens = %d (at least 1)", n_tokens);
    L2Z_CHECK(w->is_q8(), L2Z_ERR_INVALID,
              "l2z_prefill_q8: takes int8 group-quantized weights (l2z_weights_init_q8); f32 and packed weights go to l2z_prefill");
    L2Z_TRY(check_pair(config, s, w, false, true));   // (a sharded or paged runstate, another config)
    const int hs = s->sh.hs;
    L2Z_CHECK(hs % 4 == 0 && hs <= 256 && s->sh.kvd_loc % 4 == 0, L2Z_ERR_INVALID,
              "l2z_prefill_q8: needs a head_size that is a multiple of 4, at most 256");
    L2Z_TRY(check_positions("l2z_prefill_q8", "", "positions", pos0, n_tokens, config->seq_len));
    L2Z_TRY(check_tokens("l2z_prefill_q8", "", tokens, n_tokens, config->vocab_size));
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
    hipStream_t st = s->stream;
    RaggedSeq seq = {};
    seq.kc = s->key_cache; seq.vc = s->value_cache;
    L2Z_HIP(hipMemcpyAsync(b.seq, &seq, sizeof seq, hipMemcpyHostToDevice, st));
    for (int done = 0; done < n_tokens;) {
        const int P = prefill_next_chunk_of(*config, n_tokens - done);
        L2Z_TRY(q8_chunk(s, w, b, tokens + done, P, pos0 + done));
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

// The step on int8 group-quantized weights.  Per layer q | k | v in one launch (RoPE and the cache rows in
// its epilogue) and the caller's attention; then the classifier through the table.  Every product is the one-tile form of
// q8_gemm_device.h: a row's bits do not depend on n, on the other rows, or on its place in the batch.
int l2z::batch_step_q8(int n, const l2z_config &c, l2z_runstate *s0, const l2z_weights *w, BatchScratch *b, LayerAttention attention)
{
    hipStream_t st = s0->stream;
    const int dim = c.dim, hs = dim / c.n_heads, kvd = hs * c.n_kv_heads, gs = w->q8_gs;
    const BatchTable *tab = b->d_tab;
    const Q8Rows r = {n, b->x, b->att, b->h1, b->ld_att, b->ld_h1, b->q8_xq, b->q8_xs, gs, st};
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

// ---------------------------------------------------------------------------
// The pass's two launches on their own (host pointers, synchronous)
namespace {
struct DevBytes {
    void *p = nullptr;
    ~DevBytes() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { L2Z_HIP(hipMalloc(&p, bytes ? bytes : 1)); return L2Z_OK; }
};
}  // namespace

extern "C" int l2z_q8_quantize_rows(const float *x, int m, size_t n, const float *rms_w, int gs, int8_t *out_q, float *out_s)
{
    L2Z_CHECK(x && out_q && out_s && m > 0 && m <= (1 << 20) && n > 0 && n < (1u << 24), L2Z_ERR_INVALID, "l2z_q8_quantize_rows: bad arguments");
    L2Z_CHECK((gs == 32 || gs == 64) && n % (size_t)gs == 0, L2Z_ERR_INVALID,
              "l2z_q8_quantize_rows: group size %d (32 or 64, dividing n = %zu)", gs, n);
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const size_t mp = (size_t)q8_gemm_rows_padded(m), ng = n / (size_t)gs;
    DevBytes dx, dw, dq, ds;
    L2Z_TRY(dx.alloc((size_t)m * n * 4)); L2Z_TRY(dw.alloc(n * 4)); L2Z_TRY(dq.alloc(mp * n)); L2Z_TRY(ds.alloc(mp * ng * 4));
    L2Z_HIP(hipMemcpy(dx.p, x, (size_t)m * n * 4, hipMemcpyHostToDevice));
    if (rms_w) L2Z_HIP(hipMemcpy(dw.p, rms_w, n * 4, hipMemcpyHostToDevice));
    L2Z_HIP(launch_q8_quantize_rows((const float *)dx.p, (int)n, m, (int)n, rms_w ? (const float *)dw.p : nullptr, gs, (int8_t *)dq.p,
                                    (float *)ds.p, nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    L2Z_HIP(hipMemcpy(out_q, dq.p, (size_t)m * n, hipMemcpyDeviceToHost));
    L2Z_HIP(hipMemcpy(out_s, ds.p, (size_t)m * ng * 4, hipMemcpyDeviceToHost));
    return L2Z_OK;
}

extern "C" int l2z_q8_gemm(float *out, const int8_t *xq, const float *xs, int m, const int8_t *wq, const float *ws, size_t n,
                           size_t d, int gs)
{
    L2Z_CHECK(out && xq && xs && wq && ws && m > 0 && m <= (1 << 20) && n > 0 && d > 0 && n < (1u << 24) && d < (1u << 24),
              L2Z_ERR_INVALID, "l2z_q8_gemm: bad arguments");
    L2Z_CHECK((gs == 32 || gs == 64) && n % (size_t)gs == 0, L2Z_ERR_INVALID,
              "l2z_q8_gemm: group size %d (32 or 64, dividing n = %zu)", gs, n);
    L2Z_CHECK(d % 4 == 0, L2Z_ERR_INVALID, "l2z_q8_gemm: d = %zu (a multiple of 4: a lane stores four features)", d);
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const size_t mp = (size_t)q8_gemm_rows_padded(m), ng = n / (size_t)gs;
    DevBytes dxq, dxs, dwq, dws, dout;
    L2Z_TRY(dxq.alloc(mp * n)); L2Z_TRY(dxs.alloc(mp * ng * 4)); L2Z_TRY(dwq.alloc(d * n)); L2Z_TRY(dws.alloc(d * ng * 4));
    L2Z_TRY(dout.alloc((size_t)m * d * 4));
    // the rows stand padded to whole tiles, the pad rows zero, as the row launch leaves them
    L2Z_HIP(hipMemset(dxq.p, 0, mp * n));
    L2Z_HIP(hipMemset(dxs.p, 0, mp * ng * 4));
    L2Z_HIP(hipMemcpy(dxq.p, xq, (size_t)m * n, hipMemcpyHostToDevice));
    L2Z_HIP(hipMemcpy(dxs.p, xs, (size_t)m * ng * 4, hipMemcpyHostToDevice));
    L2Z_HIP(hipMemcpy(dwq.p, wq, d * n, hipMemcpyHostToDevice));
    L2Z_HIP(hipMemcpy(dws.p, ws, d * ng * 4, hipMemcpyHostToDevice));
    Q8GemmArgs a = {};
    a.xq = (const int8_t *)dxq.p; a.xs = (const float *)dxs.p; a.wq = (const int8_t *)dwq.p; a.ws = (const float *)dws.p;
    a.out = (float *)dout.p; a.ldo = (int)d;
    a.m = m; a.n = (int)n; a.d = (int)d; a.gs = gs;
    L2Z_HIP(launch_q8_gemm(a, EPI_STORE, nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    L2Z_HIP(hipMemcpy(out, dout.p, (size_t)m * d * 4, hipMemcpyDeviceToHost));
    return L2Z_OK;
}
