// kv8_host.cpp -- host side of the int8 KV cache beside wide_host.cpp's l2z_transformer_wide_q8 and runstate.cpp's
// l2z_runstate_init_kv8 / l2z_runstate_read_kv8 (include/llama2_hip_test.h): the rows l2z_runstate_fork
// puts into such a runstate, the tables the prompt attention's row form reads (l2z_prefill_kv8, q8_host.cpp; DESIGN.md
// 4.29), and the hooks that run the decode attention's two launches, the prompt attention and the verify attention (DESIGN.md
// 4.31) on their own.
#include <algorithm>
#include <cstring>
#include <vector>

#include "batch_host.h"
#include "kv8.h"
#include "kv8_layout.h"

using namespace l2z;

int l2z::kv8_fork_rows(l2z_runstate *dst, const l2z_runstate *src, int n_pos)
{
    const l2z_config &c = src->cfg;
    const size_t hs = (size_t)src->sh.hs, S = (size_t)c.seq_len, runs = (size_t)c.n_layers * c.n_kv_heads;
    hipStream_t st = dst->stream;
    if (!src->is_kv8()) {   // f32 rows (RoPE is in the keys already): the scatter's slice function over rows 0 .. n_pos - 1
        L2Z_HIP(launch_kv8_quantize_cache(src->key_cache, dst->k8, dst->ks8, (int)runs, c.seq_len, (int)hs, n_pos, st));
        L2Z_HIP(launch_kv8_quantize_cache(src->value_cache, dst->v8, dst->vs8, (int)runs, c.seq_len, (int)hs, n_pos, st));
        return L2Z_OK;
    }
    // bytes and scales: one run of n_pos rows per (layer, kv head), seq_len rows apart
    L2Z_HIP(hipMemcpy2DAsync(dst->k8, S * hs, src->k8, S * hs, (size_t)n_pos * hs, runs, hipMemcpyDeviceToDevice, st));
    L2Z_HIP(hipMemcpy2DAsync(dst->v8, S * hs, src->v8, S * hs, (size_t)n_pos * hs, runs, hipMemcpyDeviceToDevice, st));
    L2Z_HIP(hipMemcpy2DAsync(dst->ks8, S * 4, src->ks8, S * 4, (size_t)n_pos * 4, runs, hipMemcpyDeviceToDevice, st));
    L2Z_HIP(hipMemcpy2DAsync(dst->vs8, S * 4, src->vs8, S * 4, (size_t)n_pos * 4, runs, hipMemcpyDeviceToDevice, st));
    return L2Z_OK;
}

void l2z::kv8_prompt_tables(void *host, const Kv8Seq &seq, int pos0, int P, bool with_rows)
{
    memset(host, 0, kv8_prompt_table_bytes(P, with_rows));
    Kv8Seq *slots = (Kv8Seq *)host;
    std::fill(slots, slots + kWideMax, seq);
    if (!with_rows) return;
    WideTable *tab = (WideTable *)(slots + kWideMax);
    for (int r = 0; r < P; r++) tab[r / kWideMax].pos[r % kWideMax] = pos0 + r;
}

// PREVIEW (include/llama2_hip_test.h): launch_kv8_attention on its own -- host pointers, synchronous, one layer
extern "C" int l2z_kv8_attention(float *out, const float *q, const int32_t *pos, int n, const int8_t *k8, const float *ks,
                                 const int8_t *v8, const float *vs, int n_heads, int n_kv_heads, int head_size, int seq_len)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out && q && pos && k8 && ks && v8 && vs, L2Z_ERR_INVALID, "l2z_kv8_attention: null argument");
    L2Z_CHECK(n >= 1 && n <= kWideMax, L2Z_ERR_INVALID, "l2z_kv8_attention: n = %d outside [1, %d]", n, kWideMax);
    L2Z_CHECK(kv8::head_size_ok(head_size) && n_heads >= 1 && n_kv_heads >= 1 && n_heads % n_kv_heads == 0 && seq_len >= 1 &&
                  seq_len <= (1 << 20) && n_heads <= (1 << 12),
              L2Z_ERR_INVALID, "l2z_kv8_attention: head_size %d (a multiple of 4, at most 256), %d heads on %d kv heads, seq_len %d",
              head_size, n_heads, n_kv_heads, seq_len);
    int deepest = 0;
    for (int i = 0; i < n; i++) {
        L2Z_CHECK(pos[i] >= 0 && pos[i] < seq_len, L2Z_ERR_STATE, "l2z_kv8_attention: pos[%d] = %d outside [0, %d)", i, pos[i], seq_len);
        deepest = std::max(deepest, pos[i]);
    }
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const size_t hs = (size_t)head_size, S = (size_t)seq_len, dim = (size_t)n_heads * hs;
    const size_t row_s = (size_t)n_kv_heads * S, row_v = row_s * hs;   // one row's scales, values
    HookBuf<void> dq, dout, dk, dv, dks, dvs, dtab, dseq, dpart;
    L2Z_TRY(dq.put(q, (size_t)n * dim * 4)); L2Z_TRY(dout.put(nullptr, (size_t)n * dim * 4));
    L2Z_TRY(dk.put(k8, (size_t)n * row_v)); L2Z_TRY(dv.put(v8, (size_t)n * row_v));
    L2Z_TRY(dks.put(ks, (size_t)n * row_s * 4)); L2Z_TRY(dvs.put(vs, (size_t)n * row_s * 4));
    std::vector<WideTable> tab(1);
    std::vector<Kv8Seq> seq((size_t)n);
    for (int i = 0; i < n; i++) {
        tab[0].pos[i] = pos[i];
        seq[(size_t)i] = {(int8_t *)dk.p.get() + i * row_v, (int8_t *)dv.p.get() + i * row_v, (float *)dks.p.get() + i * row_s, (float *)dvs.p.get() + i * row_s};
    }
    L2Z_TRY(dtab.put(tab.data(), sizeof(WideTable)));
    L2Z_TRY(dseq.put(seq.data(), seq.size() * sizeof(Kv8Seq)));
    const int seg_cap = verify_segments(seq_len);
    L2Z_TRY(dpart.put(nullptr, wide_part_floats(n_heads, seg_cap, head_size) * 4));
    const WideAttn wa = {(const WideTable *)dtab.p.get(), (float *)dpart.p.get(), seg_cap, deepest / kVerifySeg + 1, 0, n, 0};
    const RaggedLayer L = {(const float *)dq.p.get(), (int)dim, (float *)dout.p.get(), (int)dim, n, n_heads, head_size, n_heads / n_kv_heads, seq_len,
                           0, S * hs, nullptr, nullptr, 0};
    L2Z_HIP(launch_kv8_attention(L, wa, (const Kv8Seq *)dseq.p.get()));
    L2Z_HIP(hipDeviceSynchronize());
    L2Z_HIP(hipMemcpy(out, dout.p.get(), (size_t)n * dim * 4, hipMemcpyDeviceToHost));
    return L2Z_OK;
}

// PREVIEW (include/llama2_hip_test.h): launch_kv8_prefill_attention on its own -- host pointers, synchronous, one layer, one
// sequence
extern "C" int l2z_kv8_prefill_attention(int form, float *out, const float *q, int pos0, int P, const int8_t *k8, const float *ks,
                                         const int8_t *v8, const float *vs, int n_heads, int n_kv_heads, int head_size, int seq_len)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out && q && k8 && ks && v8 && vs, L2Z_ERR_INVALID, "l2z_kv8_prefill_attention: null argument");
    L2Z_CHECK(kv8::head_size_ok(head_size) && n_heads >= 1 && n_kv_heads >= 1 && n_heads % n_kv_heads == 0 && seq_len >= 1 &&
                  seq_len <= (1 << 20) && n_heads <= (1 << 12),
              L2Z_ERR_INVALID, "l2z_kv8_prefill_attention: head_size %d (a multiple of 4, at most 256), %d heads on %d kv heads, seq_len %d",
              head_size, n_heads, n_kv_heads, seq_len);
    L2Z_CHECK(P >= 1, L2Z_ERR_INVALID, "l2z_kv8_prefill_attention: P = %d (at least 1)", P);
    L2Z_CHECK(form == 0 || form == 1 || (form == 3 && kv8_prefill_flash_shape(head_size, P)), L2Z_ERR_INVALID,
              "l2z_kv8_prefill_attention: form %d (0 by shape, 1 the row form, 3 the matrix-core form: head_size 64 or 128 and more "
              "than 32 rows; head_size %d, %d rows)", form, head_size, P);
    L2Z_TRY(check_positions("l2z_kv8_prefill_attention", "", "positions", pos0, P, seq_len));
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const size_t hs = (size_t)head_size, S = (size_t)seq_len, dim = (size_t)n_heads * hs, row_s = (size_t)n_kv_heads * S;
    const bool with_rows = form == 1 || !kv8_prefill_flash_shape(head_size, P);
    HookBuf<void> dq, dout, dk, dv, dks, dvs, dtab, dpart;
    L2Z_TRY(dq.put(q, (size_t)P * dim * 4)); L2Z_TRY(dout.put(nullptr, (size_t)P * dim * 4));
    L2Z_TRY(dk.put(k8, row_s * hs)); L2Z_TRY(dv.put(v8, row_s * hs));
    L2Z_TRY(dks.put(ks, row_s * 4)); L2Z_TRY(dvs.put(vs, row_s * 4));
    Kv8Prompt pr = {};
    pr.seq = {(int8_t *)dk.p.get(), (int8_t *)dv.p.get(), (float *)dks.p.get(), (float *)dvs.p.get()};
    std::vector<uint8_t> tab(kv8_prompt_table_bytes(P, with_rows));
    kv8_prompt_tables(tab.data(), pr.seq, pos0, P, with_rows);
    L2Z_TRY(dtab.put(tab.data(), tab.size()));
    pr.slots = (const Kv8Seq *)dtab.p.get();
    pr.tab = (const WideTable *)(pr.slots + kWideMax);
    pr.seg_cap = verify_segments(seq_len);
    if (with_rows) {
        L2Z_TRY(dpart.put(nullptr, wide_part_floats(n_heads, pr.seg_cap, head_size) * 4));
        pr.part = (float *)dpart.p.get();
    }
    L2Z_HIP(launch_kv8_prefill_attention((const float *)dq.p.get(), (int)dim, pr, (float *)dout.p.get(), (int)dim, pos0, P, n_heads, head_size,
                                         n_heads / n_kv_heads, seq_len, 0, S * hs, nullptr, form));
    L2Z_HIP(hipDeviceSynchronize());
    L2Z_HIP(hipMemcpy(out, dout.p.get(), (size_t)P * dim * 4, hipMemcpyDeviceToHost));
    return L2Z_OK;
}

// PREVIEW (include/llama2_hip_test.h): launch_kv8_verify_attention on its own -- host pointers, synchronous, one
// layer, one sequence; the layouts are l2z_kv8_prefill_attention's
extern "C" int l2z_kv8_verify_attention(float *out, const float *q, int pos0, int n, const int8_t *k8, const float *ks,
                                        const int8_t *v8, const float *vs, int n_heads, int n_kv_heads, int head_size, int seq_len)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out && q && k8 && ks && v8 && vs, L2Z_ERR_INVALID, "l2z_kv8_verify_attention: null argument");
    L2Z_CHECK(n >= 1 && n <= kBatchMax, L2Z_ERR_INVALID, "l2z_kv8_verify_attention: n = %d outside [1, %d]", n, kBatchMax);
    L2Z_CHECK(kv8::head_size_ok(head_size) && n_heads >= 1 && n_kv_heads >= 1 && n_heads % n_kv_heads == 0 && seq_len >= 1 &&
                  seq_len <= (1 << 20) && n_heads <= (1 << 12),
              L2Z_ERR_INVALID, "l2z_kv8_verify_attention: head_size %d (a multiple of 4, at most 256), %d heads on %d kv heads, seq_len %d",
              head_size, n_heads, n_kv_heads, seq_len);
    L2Z_TRY(check_positions("l2z_kv8_verify_attention", "", "positions", pos0, n, seq_len));
    L2Z_TRY(ensure_device(current_device_for(nullptr)));
    const size_t hs = (size_t)head_size, S = (size_t)seq_len, dim = (size_t)n_heads * hs, row_s = (size_t)n_kv_heads * S;
    HookBuf<void> dq, dout, dk, dv, dks, dvs, dtab, dpart;
    L2Z_TRY(dq.put(q, (size_t)n * dim * 4)); L2Z_TRY(dout.put(nullptr, (size_t)n * dim * 4));
    L2Z_TRY(dk.put(k8, row_s * hs)); L2Z_TRY(dv.put(v8, row_s * hs));
    L2Z_TRY(dks.put(ks, row_s * 4)); L2Z_TRY(dvs.put(vs, row_s * 4));
    const Kv8Seq seq = {(int8_t *)dk.p.get(), (int8_t *)dv.p.get(), (float *)dks.p.get(), (float *)dvs.p.get()};
    std::vector<uint8_t> tab(kv8_prompt_table_bytes(n, true));   // the slots, then the table whose pos[] the combine reads
    kv8_prompt_tables(tab.data(), seq, pos0, n, true);
    L2Z_TRY(dtab.put(tab.data(), tab.size()));
    const Kv8Seq *slots = (const Kv8Seq *)dtab.p.get();
    const int seg_cap = verify_segments(seq_len);
    L2Z_TRY(dpart.put(nullptr, wide_part_floats(n_heads, seg_cap, head_size) * 4));
    const WideAttn wa = {(const WideTable *)(slots + kWideMax), (float *)dpart.p.get(), seg_cap, (pos0 + n - 1) / kVerifySeg + 1, 0, 1, 0};
    const RaggedLayer L = {(const float *)dq.p.get(), (int)dim, (float *)dout.p.get(), (int)dim, n, n_heads, head_size, n_heads / n_kv_heads, seq_len,
                           0, S * hs, nullptr, nullptr, 0};
    L2Z_HIP(launch_kv8_verify_attention(L, wa, slots, 0, pos0));
    L2Z_HIP(hipDeviceSynchronize());
    L2Z_HIP(hipMemcpy(out, dout.p.get(), (size_t)n * dim * 4, hipMemcpyDeviceToHost));
    return L2Z_OK;
}
