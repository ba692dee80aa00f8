// hooks.cpp -- kernel-level entry points of include/llama2_hip_test.h (tests, and the reference's own
// unit-test shapes).  What runs behind each hook:
//   l2z_matmul / l2z_matmul_fused   launch_matvec: the forward pass's own kernels for that width
//   l2z_rmsnorm                     the mat-vec prologue's staging code (xload_issue / xstage_finish)
//   l2z_attention_decode            the forward pass's attention kernels, every form selectable
//   l2z_prefill_attention           the batched prefill's attention kernels, every form selectable
//   l2z_softmax, l2z_vector_dot_product, l2z_vector_weighted_sum_rows
//                                   the GENERIC attention kernel's device functions (block_softmax,
//                                   attn_scores, attn_weighted_sum) -- the forms the stories / 7B
//                                   shapes run are covered by l2z_attention_decode instead
//   l2z_q8_quantize, l2z_q8_matmul, l2z_q8_matvec_case
//                                   launch_q8_quantize / launch_q8_matvec: the int8 pass's own kernels, the last with
//                                   every argument of the launch the caller's
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "l2z_state.h"

using namespace l2z;

// ---------------------------------------------------------------------------
// Kernel-level test hooks: upload, launch, download.
namespace {
struct DevBuf {
    float *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) { L2Z_HIP(hipMalloc(&p, (n ? n : 1) * sizeof(float))); return L2Z_OK; }
    int up(const float *h, size_t n) { L2Z_HIP(hipMemcpy(p, h, n * sizeof(float), hipMemcpyHostToDevice)); return L2Z_OK; }
    int down(float *h, size_t n) { L2Z_HIP(hipMemcpy(h, p, n * sizeof(float), hipMemcpyDeviceToHost)); return L2Z_OK; }
};
}  // namespace

extern "C" int l2z_matmul_fused(int N, float *const *outs, const float *x, const float *const *ws,
                                size_t n, size_t d)
{
    L2Z_CHECK(N >= 1 && N <= kMaxSeg && outs && x && ws && n > 0 && d > 0, L2Z_ERR_INVALID,
              "l2z_matmul_fused: bad arguments");
    L2Z_CHECK(n < (1u << 30) && d < (1u << 30), L2Z_ERR_INVALID, "l2z_matmul_fused: too large");
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    DevBuf dx, dw[kMaxSeg], dout[kMaxSeg];
    L2Z_TRY(dx.alloc(n));
    L2Z_TRY(dx.up(x, n));
    MatvecArgs a = {};
    a.n = (int)n; a.x = dx.p;
    for (int j = 0; j < N; j++) {
        L2Z_TRY(dw[j].alloc(n * d));
        L2Z_TRY(dw[j].up(ws[j], n * d));
        L2Z_TRY(dout[j].alloc(d));
    }
    a.w0 = dw[0].p; a.out0 = dout[0].p; a.rows0 = (int)d;
    if (N > 1) { a.w1 = dw[1].p; a.out1 = dout[1].p; a.rows1 = (int)d; }
    if (N > 2) { a.w2 = dw[2].p; a.out2 = dout[2].p; a.rows2 = (int)d; }
    L2Z_HIP(launch_matvec(a, PRO_NONE, EPI_STORE, 8, g_cus, nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    for (int j = 0; j < N; j++) L2Z_TRY(dout[j].down(outs[j], d));
    return L2Z_OK;
}

extern "C" int l2z_matmul(float *xout, const float *x, const float *w, size_t n, size_t d)
{
    float *outs[1] = {xout};
    const float *ws[1] = {w};
    return l2z_matmul_fused(1, outs, x, ws, n, d);
}

extern "C" int l2z_rmsnorm(float *o, const float *x, const float *w, size_t n)
{
    L2Z_CHECK(o && x && w && n > 0 && n < (1u << 30), L2Z_ERR_INVALID, "l2z_rmsnorm: bad arguments");
    L2Z_CHECK(matvec_lds_bytes((int)n) <= 160 * 1024, L2Z_ERR_INVALID, "l2z_rmsnorm: n too large for LDS");
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    DevBuf dx, dw, dout;
    L2Z_TRY(dx.alloc(n)); L2Z_TRY(dw.alloc(n)); L2Z_TRY(dout.alloc(n));
    L2Z_TRY(dx.up(x, n)); L2Z_TRY(dw.up(w, n));
    L2Z_HIP(launch_rmsnorm(dout.p, dx.p, dw.p, (int)n, nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    return dout.down(o, n);
}

extern "C" int l2z_softmax(float *x, size_t n)
{
    L2Z_CHECK(x && n > 0 && n < (1u << 30), L2Z_ERR_INVALID, "l2z_softmax: bad arguments");
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    DevBuf dx;
    L2Z_TRY(dx.alloc(n)); L2Z_TRY(dx.up(x, n));
    L2Z_HIP(launch_softmax(dx.p, (int)n, nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    return dx.down(x, n);
}

extern "C" int l2z_vector_dot_product(float *out, const float *x, const float *y, size_t n)
{
    L2Z_CHECK(out && x && y && n > 0 && n < (1u << 30), L2Z_ERR_INVALID, "l2z_vector_dot_product: bad arguments");
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    DevBuf dx, dy, dout;
    L2Z_TRY(dx.alloc(n)); L2Z_TRY(dy.alloc(n)); L2Z_TRY(dout.alloc(1));
    L2Z_TRY(dx.up(x, n)); L2Z_TRY(dy.up(y, n));
    L2Z_HIP(launch_dot(dout.p, dx.p, dy.p, (int)n, nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    return dout.down(out, 1);
}

extern "C" int l2z_vector_weighted_sum_rows(float *xout, size_t xout_len, const float *rows,
                                            size_t rows_len, size_t row_stride,
                                            const float *weights, size_t n_weights)
{
    L2Z_CHECK(xout && rows && weights && xout_len > 0 && n_weights > 0, L2Z_ERR_INVALID,
              "l2z_vector_weighted_sum_rows: bad arguments");
    // main.zig:660-661 asserts
    L2Z_CHECK(row_stride >= xout_len && rows_len >= (n_weights - 1) * row_stride + xout_len,
              L2Z_ERR_INVALID, "l2z_vector_weighted_sum_rows: stride/length contract violated");
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    DevBuf dr, dw, dout;
    L2Z_TRY(dr.alloc(rows_len)); L2Z_TRY(dw.alloc(n_weights)); L2Z_TRY(dout.alloc(xout_len));
    L2Z_TRY(dr.up(rows, rows_len)); L2Z_TRY(dw.up(weights, n_weights));
    L2Z_HIP(launch_weighted_sum_rows(dout.p, (int)xout_len, dr.p, (int)row_stride, dw.p,
                                     (int)n_weights, nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    return dout.down(xout, xout_len);
}

extern "C" int l2z_argmax_host(const float *x, size_t n, size_t *out_index)
{
    L2Z_CHECK(x && out_index && n > 0 && n < (1u << 30), L2Z_ERR_INVALID, "l2z_argmax_host: bad arguments");
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    DevBuf dx;
    int *didx = nullptr;
    L2Z_TRY(dx.alloc(n)); L2Z_TRY(dx.up(x, n));
    L2Z_HIP(hipMalloc(&didx, sizeof(int)));
    ArgmaxArgs a = {};
    a.logits = dx.p; a.vocab = (int)n; a.argmax_out = didx; a.advance = 0;
    hipError_t e = launch_argmax(a, nullptr);
    int idx = 0;
    if (e == hipSuccess) e = hipMemcpy(&idx, didx, sizeof(int), hipMemcpyDeviceToHost);
    (void)hipFree(didx);
    L2Z_HIP(e);
    *out_index = (size_t)idx;
    return L2Z_OK;
}

// The reference's cache order (seq_len, kv_dim) (main.zig:354) -> the device's head-major order
// [kv head][seq_len][head_size], so that the hooks drive the kernels on the layout the forward
// pass gives them.
static std::vector<float> to_head_major(const float *src, int seq_len, int n_kv_heads, int head_size)
{
    const size_t kvd = (size_t)n_kv_heads * head_size;
    std::vector<float> out((size_t)seq_len * kvd);
    for (int h = 0; h < n_kv_heads; h++)
        for (int t = 0; t < seq_len; t++)
            memcpy(out.data() + ((size_t)h * seq_len + t) * head_size, src + (size_t)t * kvd + (size_t)h * head_size,
                   (size_t)head_size * sizeof(float));
    return out;
}

// src/main.zig:361-389 for the P queries of a prompt chunk at positions pos0 .. pos0 + P - 1, through the
// batched prefill's attention kernels (prefill_attention.hip).  form: 0 as l2z_prefill picks, 1 block per
// (head, query), 2 tiled with the softmax in LDS, 3 flash form (head sizes 64 and 128).
extern "C" int l2z_prefill_attention(int form, float *out, const float *q, const float *kcache, const float *vcache,
                                     int pos0, int n_queries, int n_heads, int n_kv_heads, int head_size, int seq_len)
{
    L2Z_CHECK(out && q && kcache && vcache && n_heads > 0 && n_kv_heads > 0 && head_size > 0 && head_size % 4 == 0 &&
                  n_heads % n_kv_heads == 0 && n_queries > 0 && pos0 >= 0 && pos0 + n_queries <= seq_len,
              L2Z_ERR_INVALID, "l2z_prefill_attention: bad arguments");
    L2Z_CHECK(form >= 0 && form <= 3, L2Z_ERR_INVALID, "l2z_prefill_attention: form %d", form);
    L2Z_CHECK(form < 3 || head_size == 64 || head_size == 128, L2Z_ERR_INVALID,
              "l2z_prefill_attention: the flash form takes head sizes 64 and 128");
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const size_t dim = (size_t)n_heads * head_size, kvd = (size_t)n_kv_heads * head_size;
    DevBuf dq, dk, dv, dout;
    L2Z_TRY(dq.alloc(n_queries * dim)); L2Z_TRY(dk.alloc(seq_len * kvd)); L2Z_TRY(dv.alloc(seq_len * kvd));
    L2Z_TRY(dout.alloc(n_queries * dim));
    const std::vector<float> hk = to_head_major(kcache, seq_len, n_kv_heads, head_size),
                             hv = to_head_major(vcache, seq_len, n_kv_heads, head_size);
    L2Z_TRY(dq.up(q, n_queries * dim)); L2Z_TRY(dk.up(hk.data(), seq_len * kvd)); L2Z_TRY(dv.up(hv.data(), seq_len * kvd));
    const hipError_t e = launch_prefill_attention(dq.p, (int)dim, dk.p, dv.p, dout.p, (int)dim, pos0, n_queries, n_heads,
                                                  head_size, head_size, (size_t)seq_len * head_size, n_heads / n_kv_heads,
                                                  seq_len, nullptr, n_heads, form);
    L2Z_HIP(e);
    L2Z_HIP(hipDeviceSynchronize());
    L2Z_TRY(dout.down(out, n_queries * dim));
    return L2Z_OK;
}

// src/main.zig:361-389 for one layer, through the forward pass's attention kernels
extern "C" int l2z_attention_decode(int form, int nch, float *out, const float *q, const float *kcache,
                                    const float *vcache, int pos, int n_heads, int n_kv_heads,
                                    int head_size, int seq_len)
{
    L2Z_CHECK(out && q && kcache && vcache && n_heads > 0 && n_kv_heads > 0 && head_size > 0 &&
                  n_heads % n_kv_heads == 0 && seq_len > 0 && pos >= 0 && pos < seq_len,
              L2Z_ERR_INVALID, "l2z_attention_decode: bad arguments");
    L2Z_CHECK(form >= 0 && form <= 4, L2Z_ERR_INVALID, "l2z_attention_decode: form %d", form);
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const size_t dim = (size_t)n_heads * head_size, kvd = (size_t)n_kv_heads * head_size;
    const size_t kvn = (size_t)seq_len * kvd;
    DevBuf dq, dk, dv, dout, dpart;
    int *dpos = nullptr, *dcnt = nullptr;
    L2Z_TRY(dq.alloc(dim)); L2Z_TRY(dk.alloc(kvn)); L2Z_TRY(dv.alloc(kvn)); L2Z_TRY(dout.alloc(dim));
    const std::vector<float> hk = to_head_major(kcache, seq_len, n_kv_heads, head_size),
                             hv = to_head_major(vcache, seq_len, n_kv_heads, head_size);
    L2Z_TRY(dq.up(q, dim)); L2Z_TRY(dk.up(hk.data(), kvn)); L2Z_TRY(dv.up(hv.data(), kvn));
    AttnArgs a = {};
    a.q = dq.p; a.kcache = dk.p; a.vcache = dv.p; a.xb = dout.p;
    a.head_size = head_size; a.kv_row = head_size; a.kv_head = (size_t)seq_len * head_size;
    a.kv_mul = n_heads / n_kv_heads; a.seq_len = seq_len;
    const bool fast_ok = attention_split_supported(a);  // same conditions as the fast kernels
    L2Z_CHECK(form == 0 || form == 4 || fast_ok, L2Z_ERR_INVALID,
              "l2z_attention_decode: form %d needs head_size %% 4 == 0 and <= 256", form);
    const size_t att_lds = attention_lds_bytes(head_size, seq_len, fast_ok);
    L2Z_CHECK(att_lds <= 160 * 1024, L2Z_ERR_INVALID, "l2z_attention_decode: seq_len too long for LDS");
    hipError_t e = hipMalloc(&dpos, sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(dpos, &pos, sizeof(int), hipMemcpyHostToDevice);
    a.pos_ptr = dpos;
    int use_nch = 0;
    if (e == hipSuccess && (form == 3 || (form == 0 && fast_ok && pos >= 256 && seq_len > 256))) {
        use_nch = nch > 0 ? nch : attention_split_chunks(n_heads, g_cus);
        if (use_nch > 16) use_nch = 16;
        if (use_nch < 2) use_nch = form == 3 ? 2 : 0;
    }
    if (e == hipSuccess && use_nch > 1) {
        int rc = dpart.alloc(attention_split_part_floats(n_heads, head_size, use_nch));
        if (rc != L2Z_OK) { (void)hipFree(dpos); return rc; }
        e = hipMalloc(&dcnt, (size_t)n_heads * sizeof(int));
        if (e == hipSuccess) e = hipMemset(dcnt, 0, (size_t)n_heads * sizeof(int));
        // twice: the second launch finds the counters as the first one left them
        const bool small = pos < attention_split_wide_pos(seq_len);  // as the forward pass picks at this position
        if (e == hipSuccess) e = launch_attention_split(a, n_heads, use_nch, dpart.p, dcnt, nullptr, small);
        if (e == hipSuccess) e = launch_attention_split(a, n_heads, use_nch, dpart.p, dcnt, nullptr, small);
    } else if (e == hipSuccess) {
        // form 0: what the forward pass launches at this position (attn_variant: the short-context form first)
        const int auto_form = pos < attention_short_pos(head_size, seq_len) ? 1 : 0;
        e = launch_attention(a, n_heads, nullptr, form == 3 || form == 0 ? auto_form : form);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(dpos);
    if (dcnt) (void)hipFree(dcnt);
    L2Z_HIP(e);
    return dout.down(out, dim);
}

extern "C" int l2z_option_set(const char *env_name, long long value)
{
    L2Z_CHECK(env_name != nullptr && tunables_set(env_name, value), L2Z_ERR_INVALID,
              "l2z_option_set: unknown option '%s'", env_name ? env_name : "(null)");
    return L2Z_OK;
}

// Host-side shard geometry (no device needed): what rank `rank` of `world` owns under scheme A (rows) and, for Wo / W2 under
// scheme B, the padded width of its column shards.  out[0..9] = dim0, dim_loc, kvd_loc, heads_loc, hid0, hid_loc, v0, v_loc,
// dimc_pad, hidc_pad.
extern "C" int l2z_shard_plan(const l2z_config *config, int rank, int world, int *out, int cap)
{
    L2Z_CHECK(config != nullptr && out != nullptr && cap >= 10 && world >= 1 && rank >= 0 && rank < world, L2Z_ERR_INVALID,
              "l2z_shard_plan: bad arguments");
    l2z_comm c;
    c.rank = rank; c.world = world; c.device = 0; c.nccl = nullptr;
    Shard sh;
    L2Z_TRY(make_shard(*config, &c, &sh));
    const int v[10] = {sh.dim0, sh.dim_loc, sh.kvd_loc, sh.heads_loc, sh.hid0, sh.hid_loc, sh.v0, sh.v_loc, sh.dimc_pad, sh.hidc_pad};
    for (int i = 0; i < 10; i++) out[i] = v[i];
    return L2Z_OK;
}

// Host-side planning of the batched prefill, no device needed: how a prompt is cut into chunks, and which
// output tile the direct-to-LDS GEMM takes for a [P, N] product (0: 128x64, 1: 64x64, 2: 32x64, 3: 32x32,
// 4: 128x128; the CU count is the current device's, 256 without one).
extern "C" int l2z_prefill_plan_model(const l2z_config *config, int n_tokens, int *chunks, int cap)
{
    L2Z_CHECK(config != nullptr && n_tokens >= 0 && (chunks != nullptr || cap == 0), L2Z_ERR_INVALID, "l2z_prefill_plan_model: bad arguments");
    L2Z_CHECK(config->n_heads > 0 && config->dim > 0, L2Z_ERR_INVALID, "l2z_prefill_plan_model: bad config");
    int n = 0;
    for (int done = 0; done < n_tokens; n++) {
        const int P = prefill_next_chunk_of(*config, n_tokens - done);
        if (n < cap) chunks[n] = P;
        done += P;
    }
    return n;
}

extern "C" int l2z_prefill_plan(int n_tokens, int *chunks, int cap)
{
    L2Z_CHECK(n_tokens >= 0 && (chunks != nullptr || cap == 0), L2Z_ERR_INVALID, "l2z_prefill_plan: bad arguments");
    int n = 0;
    for (int done = 0; done < n_tokens; n++) {
        const int P = prefill_next_chunk(n_tokens - done);
        if (n < cap) chunks[n] = P;
        done += P;
    }
    return n;
}

extern "C" int l2z_prefill_split_k(long long n_features_whole, int n_tokens, int k, int paired)
{
    L2Z_CHECK(n_features_whole > 0 && n_tokens > 0 && k > 0, L2Z_ERR_INVALID, "l2z_prefill_split_k: bad arguments");
    return prefill_split_k(n_features_whole, n_tokens, k, paired != 0);
}

extern "C" int l2z_prefill_cores(long long n_features_whole, int n_tokens, int k)
{
    L2Z_CHECK(n_features_whole > 0 && n_tokens > 0 && k > 0, L2Z_ERR_INVALID, "l2z_prefill_cores: bad arguments");
    const int kp = (k + 63) / 64 * 64;
    if (!x3_applies(n_features_whole, kp)) return 0;
    return x3_stream_shape(n_features_whole, n_tokens, kp) ? 1 + x3_stream_sk(n_features_whole, n_tokens, kp) : 1;
}

extern "C" int l2z_prefill_tile(int n_features, int n_tokens, int paired)
{
    L2Z_CHECK(n_features > 0 && n_tokens > 0, L2Z_ERR_INVALID, "l2z_prefill_tile: bad arguments");
    return prefill_tile_form(n_features, n_tokens, paired);
}

extern "C" int l2z_prefill_gemm_plan(const l2z_gemm_shape *shape, l2z_gemm_plan *plan)
{
    L2Z_CHECK(shape != nullptr && plan != nullptr, L2Z_ERR_INVALID, "l2z_prefill_gemm_plan: null argument");
    GemmShape g = {};
    g.kind = shape->kind; g.epi = shape->epi; g.P = shape->n_tokens; g.N = shape->n_features; g.K = shape->k; g.ldx = shape->ldx;
    g.n_scale = shape->n_scale; g.n_launch_whole = shape->n_launch_whole; g.sk = shape->sk; g.nq = shape->nq; g.nkv = shape->nkv;
    g.w13_one_matrix = shape->w13_one_matrix; g.part_floats = (size_t)shape->part_floats; g.cnt_ints = shape->cnt_ints;
    const GemmPlan p = prefill_gemm_plan(g);
    static_assert(sizeof(l2z_gemm_plan) == sizeof(GemmPlan), "include/llama2_hip_test.h l2z_gemm_plan");
    memcpy(plan, &p, sizeof p);
    return L2Z_OK;
}

// ---------------------------------------------------------------------------
// int8 group quantization: the activation rule on its own, and the product on its own through the
// forward pass's kernel body (its prologue takes the quantized x as it is)
extern "C" int l2z_q8_quantize(const float *x, size_t n, int gs, int8_t *out_q, float *out_s)
{
    L2Z_CHECK(x && out_q && out_s && n > 0 && n < (1u << 30), L2Z_ERR_INVALID, "l2z_q8_quantize: bad arguments");
    L2Z_CHECK((gs == 32 || gs == 64) && n % (size_t)gs == 0, L2Z_ERR_INVALID,
              "l2z_q8_quantize: group size %d (32 or 64, dividing n = %zu)", gs, n);
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    DevBuf dx, dq, ds;
    L2Z_TRY(dx.alloc(n)); L2Z_TRY(dq.alloc(n / 4)); L2Z_TRY(ds.alloc(n / gs));
    L2Z_TRY(dx.up(x, n));
    L2Z_HIP(launch_q8_quantize(dx.p, n, gs, false, (int8_t *)dq.p, ds.p, nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    L2Z_HIP(hipMemcpy(out_q, dq.p, n, hipMemcpyDeviceToHost));
    return ds.down(out_s, n / gs);
}

extern "C" int l2z_q8_matmul(float *out, const int8_t *xq, const float *xs, const int8_t *wq, const float *ws, size_t n,
                             size_t d, int gs)
{
    L2Z_CHECK(out && xq && xs && wq && ws && n > 0 && d > 0 && n < (1u << 30) && d < (1u << 30), L2Z_ERR_INVALID,
              "l2z_q8_matmul: bad arguments");
    L2Z_CHECK((gs == 32 || gs == 64) && n % (size_t)gs == 0, L2Z_ERR_INVALID,
              "l2z_q8_matmul: group size %d (32 or 64, dividing n = %zu)", gs, n);
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const size_t ng = n / gs;
    DevBuf dxq, dxs, dwq, dws, dout;
    L2Z_TRY(dxq.alloc(n / 4)); L2Z_TRY(dxs.alloc(ng)); L2Z_TRY(dwq.alloc(n * d / 4)); L2Z_TRY(dws.alloc(ng * d));
    L2Z_TRY(dout.alloc(d));
    L2Z_HIP(hipMemcpy(dxq.p, xq, n, hipMemcpyHostToDevice));
    L2Z_HIP(hipMemcpy(dwq.p, wq, n * d, hipMemcpyHostToDevice));
    L2Z_TRY(dxs.up(xs, ng)); L2Z_TRY(dws.up(ws, ng * d));
    Q8MatvecArgs a = {};
    a.gs = gs;
    a.q0 = (const int8_t *)dwq.p; a.s0 = dws.p;
    a.xq = (const int8_t *)dxq.p; a.xs = dxs.p;
    a.b.n = (int)n; a.b.rows0 = (int)d; a.b.out0 = dout.p;
    L2Z_HIP(launch_q8_matvec(a, EPI_STORE, 8, g_cus, nullptr));
    L2Z_HIP(hipDeviceSynchronize());
    return dout.down(out, d);
}

// One launch of the q8 mat-vec as the pass issues it, every argument the caller's (include/llama2_hip_test.h): the
// epilogue, up to three segments, x in any of its three forms, the RoPE table and the head-major caches, the residual in
// place or not, and the two numbers the launcher sizes its grid from.  Goes through launch_q8_matvec as it stands.
namespace {
struct DevBytes {
    void *p = nullptr;
    ~DevBytes() { if (p) (void)hipFree(p); }
    int up(const void *h, size_t bytes)
    {
        L2Z_HIP(hipMalloc(&p, bytes ? bytes : 1));
        if (h != nullptr && bytes > 0) L2Z_HIP(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
        return L2Z_OK;
    }
};
}  // namespace

extern "C" int l2z_q8_matvec_case(l2z_q8_case *c)
{
    L2Z_CHECK(c != nullptr, L2Z_ERR_INVALID, "l2z_q8_matvec_case: null argument");
    const int epi = c->epi, gs = c->gs, n = c->n;
    L2Z_CHECK(epi >= EPI_STORE && epi <= EPI_ARGMAX, L2Z_ERR_INVALID, "l2z_q8_matvec_case: epilogue %d", epi);
    L2Z_CHECK((gs == 32 || gs == 64) && n > 0 && n < (1 << 24) && n % gs == 0, L2Z_ERR_INVALID,
              "l2z_q8_matvec_case: group size %d (32 or 64, dividing n = %d)", gs, n);
    const int rows[3] = {c->rows0, c->rows1, c->rows2};
    L2Z_CHECK(rows[0] > 0 && rows[1] >= 0 && rows[2] >= 0 && rows[0] < (1 << 22) && rows[1] < (1 << 22) && rows[2] < (1 << 22) &&
                  (rows[1] > 0 || rows[2] == 0),
              L2Z_ERR_INVALID, "l2z_q8_matvec_case: rows %d, %d, %d", rows[0], rows[1], rows[2]);
    L2Z_CHECK(epi != EPI_SWIGLU || (rows[1] == rows[0] && rows[2] == 0), L2Z_ERR_INVALID,
              "l2z_q8_matvec_case: swiglu takes rows0 == rows1 pairs of one interleaved slot");
    L2Z_CHECK((epi != EPI_RESID && epi != EPI_ARGMAX) || (rows[1] == 0 && rows[2] == 0), L2Z_ERR_INVALID,
              "l2z_q8_matvec_case: resid and argmax take one segment");
    L2Z_CHECK(c->max_blocks_per_cu >= 0 && c->max_blocks_per_cu <= 8 && c->n_cus >= 0 && c->n_cus <= 4096, L2Z_ERR_INVALID,
              "l2z_q8_matvec_case: max_blocks_per_cu %d (0 .. 8), n_cus %d (0 .. 4096)", c->max_blocks_per_cu, c->n_cus);
    // the segments the launch reads (swiglu: one slot of 2 * rows0 interleaved rows), and x in exactly one form
    const int8_t *hq[3] = {c->q0, c->q1, c->q2};
    const float *hs[3] = {c->s0, c->s1, c->s2};
    const int n_seg = epi == EPI_SWIGLU ? 1 : (rows[2] > 0 ? 3 : (rows[1] > 0 ? 2 : 1));
    for (int j = 0; j < n_seg; j++)
        L2Z_CHECK(hq[j] != nullptr && hs[j] != nullptr, L2Z_ERR_INVALID, "l2z_q8_matvec_case: segment %d is null", j);
    const bool quantized = c->xq != nullptr;
    L2Z_CHECK(quantized ? (c->xs != nullptr && c->x == nullptr && c->rms_w == nullptr) : c->x != nullptr, L2Z_ERR_INVALID,
              "l2z_q8_matvec_case: x comes quantized (xq, xs) or as f32 (x, with or without rms_w)");
    // the outputs: in and out, so that what the launch must not touch can be checked
    float *ho[3] = {c->out0, c->out1, c->out2};
    const size_t olen[3] = {c->out0_len, c->out1_len, c->out2_len};
    const int n_out = epi == EPI_SWIGLU ? 1 : n_seg;
    size_t kv_head_stride = 0;
    if (epi == EPI_ROPE) {
        const int hsz = c->head_size;
        L2Z_CHECK(hsz > 0 && hsz % 2 == 0 && c->seq_len > 0 && c->pos >= 0 && c->pos < c->seq_len && c->rope != nullptr &&
                      c->rope_segs >= 0 && c->rope_segs <= 3,
                  L2Z_ERR_INVALID, "l2z_q8_matvec_case: rope: head_size %d, pos %d of seq_len %d, rope_segs %d", hsz, c->pos,
                  c->seq_len, c->rope_segs);
        // a pair (i, i + 1) never straddles two segments or two heads
        L2Z_CHECK(rows[0] % hsz == 0 && rows[1] % hsz == 0 && rows[2] % hsz == 0, L2Z_ERR_INVALID,
                  "l2z_q8_matvec_case: rope: every segment holds whole heads of %d rows", hsz);
        kv_head_stride = (size_t)c->seq_len * hsz;
    }
    for (int j = 0; j < n_out; j++) {
        size_t need = (size_t)rows[j];
        if (epi == EPI_ROPE && j > 0) need = (size_t)(rows[j] / c->head_size) * kv_head_stride;
        L2Z_CHECK(ho[j] != nullptr && olen[j] >= need, L2Z_ERR_INVALID, "l2z_q8_matvec_case: out%d holds %zu floats, the launch needs %zu",
                  j, olen[j], need);
    }
    L2Z_CHECK(epi != EPI_RESID || c->in_place || c->resid != nullptr, L2Z_ERR_INVALID, "l2z_q8_matvec_case: resid is null");
    L2Z_CHECK(epi != EPI_ARGMAX || (c->part_val != nullptr && c->part_idx != nullptr && c->part_cap > 0), L2Z_ERR_INVALID,
              "l2z_q8_matvec_case: argmax needs part_val / part_idx");
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const int n_cus = c->n_cus > 0 ? c->n_cus : g_cus;
    const int mb = c->max_blocks_per_cu > 0 ? c->max_blocks_per_cu : Tunables::max_blocks_per_cu;
    const size_t ng = (size_t)n / gs;

    DevBytes dq[3], ds[3], dxq, dxs, dx, drms, dout[3], dresid, drope, dpos, dpv, dpi;
    Q8MatvecArgs a = {};
    a.gs = gs;
    for (int j = 0; j < n_seg; j++) {
        const size_t r = epi == EPI_SWIGLU ? 2 * (size_t)rows[0] : (size_t)rows[j];
        L2Z_TRY(dq[j].up(hq[j], r * (size_t)n));
        L2Z_TRY(ds[j].up(hs[j], r * ng * sizeof(float)));
    }
    a.q0 = (const int8_t *)dq[0].p; a.q1 = (const int8_t *)dq[1].p; a.q2 = (const int8_t *)dq[2].p;
    a.s0 = (const float *)ds[0].p; a.s1 = (const float *)ds[1].p; a.s2 = (const float *)ds[2].p;
    if (quantized) {
        L2Z_TRY(dxq.up(c->xq, (size_t)n));
        L2Z_TRY(dxs.up(c->xs, ng * sizeof(float)));
        a.xq = (const int8_t *)dxq.p; a.xs = (const float *)dxs.p;
    } else {
        L2Z_TRY(dx.up(c->x, (size_t)n * sizeof(float)));
        a.b.x = (const float *)dx.p;
        if (c->rms_w != nullptr) {
            L2Z_TRY(drms.up(c->rms_w, (size_t)n * sizeof(float)));
            a.b.rms_w = (const float *)drms.p;
        }
    }
    for (int j = 0; j < n_out; j++) L2Z_TRY(dout[j].up(ho[j], olen[j] * sizeof(float)));
    a.b.out0 = (float *)dout[0].p; a.b.out1 = (float *)dout[1].p; a.b.out2 = (float *)dout[2].p;
    a.b.rows0 = rows[0]; a.b.rows1 = rows[1]; a.b.rows2 = rows[2];
    a.b.n = n;
    if (epi == EPI_ROPE) {   // as enqueue_forward_q8's q | k | v launch
        L2Z_TRY(drope.up(c->rope, (size_t)(c->pos + 1) * (size_t)(c->head_size / 2) * sizeof(float2)));
        L2Z_TRY(dpos.up(&c->pos, sizeof(int)));
        a.b.rope = (const float2 *)drope.p; a.b.pos_ptr = (const int *)dpos.p;
        a.b.head_size = c->head_size; a.b.rope_segs = c->rope_segs;
        a.b.pos_stride1 = c->head_size; a.b.pos_stride2 = c->head_size; a.b.kv_head_stride = kv_head_stride;
    }
    if (epi == EPI_RESID) {
        if (c->in_place) {   // out0 == resid, as the pass's Wo and W2 launches: the buffer starts as the residual
            a.b.resid = a.b.out0;
        } else {
            L2Z_TRY(dresid.up(c->resid, (size_t)rows[0] * sizeof(float)));
            a.b.resid = (const float *)dresid.p;
        }
    }
    if (epi == EPI_ARGMAX) {
        const size_t room = (size_t)matvec_max_grid(n_cus);   // the launcher never launches more blocks
        L2Z_TRY(dpv.up(nullptr, room * sizeof(float)));
        L2Z_TRY(dpi.up(nullptr, room * sizeof(int)));
        a.b.part_val = (float *)dpv.p; a.b.part_idx = (int *)dpi.p;
    }
    int grid = 0;
    L2Z_HIP(launch_q8_matvec(a, epi, mb, n_cus, nullptr, &grid));
    L2Z_HIP(hipDeviceSynchronize());
    c->grid = grid;
    for (int j = 0; j < n_out; j++) L2Z_HIP(hipMemcpy(ho[j], dout[j].p, olen[j] * sizeof(float), hipMemcpyDeviceToHost));
    if (epi == EPI_ARGMAX) {
        L2Z_CHECK(grid <= c->part_cap, L2Z_ERR_INVALID, "l2z_q8_matvec_case: %d candidates, room for %d", grid, c->part_cap);
        L2Z_HIP(hipMemcpy(c->part_val, dpv.p, (size_t)grid * sizeof(float), hipMemcpyDeviceToHost));
        L2Z_HIP(hipMemcpy(c->part_idx, dpi.p, (size_t)grid * sizeof(int), hipMemcpyDeviceToHost));
    }
    return L2Z_OK;
}
