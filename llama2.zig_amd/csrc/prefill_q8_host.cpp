// prefill_q8_host.cpp -- host side of l2z_prefill_q8 (include/llama2_hip_test.h): the batched prompt pass
// on int8 group-quantized weights.  A layer walk of its own, apart from prefill_host.cpp's: per layer four row launches
// (q8_rows.hip: the group quantization of the chunk's rows, after the rmsnorm where the decode's launch has one), six
// GEMM launches on the int8 matrix cores (q8_gemm.hip: q, k, v into scratch, Wo and W2 with the residual, W1 | W3 with
// SwiGLU), the f32 pass's RoPE + cache scatter over a one-sequence table and its prompt attention.  The last row then
// goes through the decode's own classifier launch, so the runstate is left as after a decode step.  Also the two hooks
// that run the row launch and the GEMM on their own.
#include <algorithm>
#include <cstring>

#include "batch_host.h"
#include "kind_rows.h"

using namespace l2z;

namespace {

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
    const int dim = c.dim, hid = c.hidden_dim, kvd = s->sh.kvd_loc, hs = s->sh.hs, gs = w->q8_gs;
    const size_t kvh_stride = (size_t)c.seq_len * hs;
    L2Z_HIP(hipMemcpyAsync(b.tokens, tokens, (size_t)P * 4, hipMemcpyHostToDevice, st));
    L2Z_HIP(launch_q8_embed_rows(w->q8_emb(), b.tokens, dim, P, b.x, pos0, b.row_seq, b.row_pos, st));
    RaggedChunk rg = {};
    rg.seq = b.seq; rg.row_seq = b.row_seq; rg.row_pos = b.row_pos;
    rg.n_seq = 1; rg.seq_max = 1; rg.k = b.k; rg.v = b.v;
    // rows of `x` (after the rmsnorm with rms_w, if any) quantized over n, then their product with the layer's matrix
    const auto rows = [&](const float *x, int n, const float *rms_w) -> int {
        L2Z_HIP(launch_q8_quantize_rows(x, n, P, n, rms_w, gs, b.xq, b.xs, st));
        return L2Z_OK;
    };
    const auto gemm = [&](const l2z_weights::Q8Mat &m, int l, int d, int n, float *out, int ldo, int epi) -> int {
        const size_t at = (size_t)l * (size_t)d * (size_t)n;
        Q8GemmArgs a = {};
        a.xq = b.xq; a.xs = b.xs; a.wq = m.q + at; a.ws = m.s + at / (size_t)gs;
        a.out = out; a.ldo = ldo; a.res = out; a.ldres = ldo;
        a.m = P; a.n = n; a.d = d; a.gs = gs;
        L2Z_HIP(launch_q8_gemm(a, epi, st));
        return L2Z_OK;
    };
    for (int l = 0; l < c.n_layers; l++) {
        const size_t layer_off = (size_t)l * c.seq_len * kvd;
        L2Z_TRY(rows(b.x, dim, w->rms_att + (size_t)l * dim));                    // :305
        L2Z_TRY(gemm(w->q_wq, l, dim, dim, b.q, dim, EPI_STORE));                 // :308-320
        L2Z_TRY(gemm(w->q_wk, l, kvd, dim, b.k, kvd, EPI_STORE));
        L2Z_TRY(gemm(w->q_wv, l, kvd, dim, b.v, kvd, EPI_STORE));
        L2Z_HIP(launch_ragged_rope_scatter(b.q, dim, rg, P, dim, kvd, hs, s->rope, layer_off, kvh_stride, st));   // :336-358
        L2Z_HIP(launch_prefill_attention(b.q, dim, s->key_cache + layer_off, s->value_cache + layer_off, b.att, dim, pos0, P,
                                         c.n_heads, hs, hs, kvh_stride, c.n_heads / c.n_kv_heads, c.seq_len, st, c.n_heads));   // :361-389
        L2Z_TRY(rows(b.att, dim, nullptr));
        L2Z_TRY(gemm(w->q_wo, l, dim, dim, b.x, dim, EPI_RESID));                 // :392-395
        L2Z_TRY(rows(b.x, dim, w->rms_ffn + (size_t)l * dim));                    // :398
        L2Z_TRY(gemm(w->q_w13, l, 2 * hid, dim, b.h, hid, EPI_SWIGLU));           // :405-416
        L2Z_TRY(rows(b.h, hid, nullptr));
        L2Z_TRY(gemm(w->q_w2, l, dim, hid, b.x, dim, EPI_RESID));                 // :419-422
    }
    return L2Z_OK;
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
