// weights_q8.cpp -- the Weights object of int8 group-quantized weights (llama2.c version-2 checkpoints):
// its allocation, the upload of a file's body, the quantization of an f32 object on the device, and the read-back.
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "l2z_state.h"
#include "q8_layout.h"

using namespace l2z;

// ---------------------------------------------------------------------------
// int8 group-quantized weights (llama2.c version-2 checkpoints; DESIGN.md 4.23, include/llama2_hip_test.h)
namespace {

// the device slots of a q8 weights object, in the order of l2z_weights' Q8Mat members; W1 and W3 share W13
enum { Q8S_EMB = 0, Q8S_WQ, Q8S_WK, Q8S_WV, Q8S_WO, Q8S_W13, Q8S_W2, Q8S_CLS, Q8S_COUNT };

struct Q8Slot {
    size_t values;   // int8 values (0: the slot is not there)
    size_t q_off, s_off;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int q8_layout_of(const char *fn, const l2z_config *c, int shared, int gs, uint64_t n_bytes, bool with_body, q8::Layout *lay)
{
    const q8::Dims d = {c->dim, c->hidden_dim, c->n_layers, c->n_heads, c->n_kv_heads, c->vocab_size, c->seq_len};
    const int st = with_body ? q8::layout_checked(d, shared != 0, gs, n_bytes, lay) : q8::layout(d, shared != 0, gs, lay);
    L2Z_CHECK(st == q8::LAYOUT_OK, L2Z_ERR_INVALID, "%s: %s (dim %d, hidden_dim %d, group_size %d, %llu bytes)", fn,
              q8::status_text(st), c->dim, c->hidden_dim, gs, (unsigned long long)n_bytes);
    return L2Z_OK;
}

// an empty q8 weights object with its allocation carved: the norm vectors, then every slot's values and scales
int q8_alloc(const l2z_config *config, int shared, int gs, const q8::Layout &lay, l2z_weights **out)
{
    const int dev = current_device_for(nullptr);
    L2Z_TRY(ensure_device(dev));
    Shard sh;
    L2Z_TRY(make_shard(*config, nullptr, &sh));   // (the dimensions l2z_transformer accepts)
    static std::atomic<uint64_t> next_uid{uint64_t(1) << 32};   // apart from weights_alloc's
    l2z_weights *w = new l2z_weights();
    w->uid = next_uid.fetch_add(1);
    w->cfg = *config;
    w->shared = shared ? 1 : 0;
    w->device = dev;
    w->sh = sh;
    w->file_layout = false;
    w->q8_gs = gs;
    const size_t L = config->n_layers, dim = config->dim;
    Q8Slot sl[Q8S_COUNT] = {};
    sl[Q8S_EMB].values = lay.t[q8::T_EMB].values();
    sl[Q8S_WQ].values = lay.t[q8::T_WQ].values();
    sl[Q8S_WK].values = lay.t[q8::T_WK].values();
    sl[Q8S_WV].values = lay.t[q8::T_WV].values();
    sl[Q8S_WO].values = lay.t[q8::T_WO].values();
    sl[Q8S_W13].values = 2 * lay.t[q8::T_W1].values();
    sl[Q8S_W2].values = lay.t[q8::T_W2].values();
    sl[Q8S_CLS].values = lay.t[q8::T_CLS].present ? lay.t[q8::T_CLS].values() : 0;
    size_t off = 0;
    const size_t o_att = off; off = align256(off + L * dim * 4);
    const size_t o_ffn = off; off = align256(off + L * dim * 4);
    const size_t o_fin = off; off = align256(off + dim * 4);
    for (auto &s : sl) {
        s.q_off = off; off = align256(off + s.values);
        s.s_off = off; off = align256(off + s.values / (size_t)gs * 4);
    }
    hipError_t e = hipMalloc((void **)&w->q8_blob, off);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) for int8 weights failed: %s", off, hipGetErrorString(e));
        delete w;
        return e == hipErrorOutOfMemory ? L2Z_ERR_OOM : L2Z_ERR_HIP;
    }
    w->rms_att = (const float *)(w->q8_blob + o_att);
    w->rms_ffn = (const float *)(w->q8_blob + o_ffn);
    w->rms_final = (const float *)(w->q8_blob + o_fin);
    l2z_weights::Q8Mat *mats[Q8S_COUNT] = {&w->q_emb, &w->q_wq, &w->q_wk, &w->q_wv, &w->q_wo, &w->q_w13, &w->q_w2, &w->q_cls};
    for (int i = 0; i < Q8S_COUNT; i++) {
        if (sl[i].values == 0) continue;
        mats[i]->q = (const int8_t *)(w->q8_blob + sl[i].q_off);
        mats[i]->s = (const float *)(w->q8_blob + sl[i].s_off);
    }
    if (sl[Q8S_CLS].values == 0) w->q_cls = w->q_emb;
    *out = w;
    return L2Z_OK;
}

// where tensor t of the file lies on the device: its slot, and for W1 / W3 which row of each interleaved pair
struct Q8Place {
    const l2z_weights::Q8Mat *m;
    int interleave;   // 0: rows contiguous; else rows 2 r + (interleave - 1)
};
Q8Place q8_place(const l2z_weights *w, int t)
{
    switch (t) {
        case q8::T_EMB: return {&w->q_emb, 0};
        case q8::T_WQ: return {&w->q_wq, 0};
        case q8::T_WK: return {&w->q_wk, 0};
        case q8::T_WV: return {&w->q_wv, 0};
        case q8::T_WO: return {&w->q_wo, 0};
        case q8::T_W1: return {&w->q_w13, 1};
        case q8::T_W2: return {&w->q_w2, 0};
        case q8::T_W3: return {&w->q_w13, 2};
        default: return {&w->q_cls, 0};
    }
}

// `layers` matrices of one file tensor between the host and the device (to_device or back): the values, then the scales
hipError_t q8_copy_tensor(const l2z_weights *w, const q8::Mat &m, int t, size_t layer0, size_t layers, int8_t *host_q,
                          float *host_s, bool to_device)
{
    const Q8Place pl = q8_place(w, t);
    const size_t gs = (size_t)w->q8_gs, row_q = m.cols, row_s = m.cols / gs * 4, rows = m.rows;
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    hipError_t e = hipSuccess;
    for (size_t l = 0; l < layers && e == hipSuccess; l++) {
        const size_t il = pl.interleave ? 2 : 1, first = pl.interleave ? (size_t)(pl.interleave - 1) : 0;
        char *dq = (char *)pl.m->q + ((layer0 + l) * rows * il + first) * row_q;
        char *ds = (char *)pl.m->s + ((layer0 + l) * rows * il + first) * row_s;
        char *hq = (char *)host_q + l * rows * row_q, *hs = (char *)host_s + l * rows * row_s;
        if (to_device) {
            e = hipMemcpy2D(dq, il * row_q, hq, row_q, row_q, rows, kind);
            if (e == hipSuccess) e = hipMemcpy2D(ds, il * row_s, hs, row_s, row_s, rows, kind);
        } else {
            e = hipMemcpy2D(hq, row_q, dq, il * row_q, row_q, rows, kind);
            if (e == hipSuccess) e = hipMemcpy2D(hs, row_s, ds, il * row_s, row_s, rows, kind);
        }
    }
    return e;
}

}  // namespace

extern "C" int l2z_weights_init_q8(const l2z_config *config, const void *body, size_t n_bytes, int shared_classifier,
                                   int group_size, const l2z_comm *comm, l2z_weights **out)
{
    L2Z_CHECK(config != nullptr && body != nullptr && out != nullptr, L2Z_ERR_INVALID, "l2z_weights_init_q8: null argument");
    L2Z_CHECK(comm == nullptr, L2Z_ERR_INVALID, "l2z_weights_init_q8: int8 group-quantized weights are unsharded (comm must be null)");
    q8::Layout lay;
    L2Z_TRY(q8_layout_of("l2z_weights_init_q8", config, shared_classifier, group_size, n_bytes, true, &lay));
    l2z_weights *w = nullptr;
    L2Z_TRY(q8_alloc(config, shared_classifier, group_size, lay, &w));
    const char *b = (const char *)body;
    const size_t L = config->n_layers, dim = config->dim;
    hipError_t e = hipMemcpy((void *)w->rms_att, b + lay.rms_att_off, L * dim * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((void *)w->rms_ffn, b + lay.rms_ffn_off, L * dim * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((void *)w->rms_final, b + lay.rms_final_off, dim * 4, hipMemcpyHostToDevice);
    for (int t = 0; t < q8::T_COUNT && e == hipSuccess; t++) {
        const q8::Mat &m = lay.t[t];
        if (!m.present) continue;
        e = q8_copy_tensor(w, m, t, 0, m.layers, (int8_t *)(b + m.q_off), (float *)(b + m.s_off), true);
    }
    if (e != hipSuccess) {
        set_error("l2z_weights_init_q8: upload failed: %s", hipGetErrorString(e));
        l2z_weights_free(w);
        return L2Z_ERR_HIP;
    }
    *out = w;
    return L2Z_OK;
}

extern "C" int l2z_weights_init_q8_from(const l2z_weights *src, int group_size, l2z_weights **out)
{
    L2Z_CHECK(src != nullptr && out != nullptr, L2Z_ERR_INVALID, "l2z_weights_init_q8_from: null argument");
    L2Z_CHECK(!src->is_q8() && src->file_layout, L2Z_ERR_INVALID,
              "l2z_weights_init_q8_from: the source must be an unsharded f32 weights object");
    q8::Layout lay;
    L2Z_TRY(q8_layout_of("l2z_weights_init_q8_from", &src->cfg, src->shared, group_size, 0, false, &lay));
    L2Z_HIP(hipSetDevice(src->device));
    l2z_weights *w = nullptr;
    L2Z_TRY(q8_alloc(&src->cfg, src->shared, group_size, lay, &w));
    const size_t L = src->cfg.n_layers, dim = src->cfg.dim;
    hipError_t e = hipMemcpy((void *)w->rms_att, src->rms_att, L * dim * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy((void *)w->rms_ffn, src->rms_ffn, L * dim * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemcpy((void *)w->rms_final, src->rms_final, dim * 4, hipMemcpyDeviceToDevice);
    // every f32 tensor is one contiguous run on the device, W1 | W3 one interleaved slot there as here: a launch a slot
    const auto quant = [&](const float *f, const l2z_weights::Q8Mat &m, size_t values) {
        if (e == hipSuccess) e = launch_q8_quantize(f, values, group_size, true, (int8_t *)m.q, (float *)m.s, nullptr);
    };
    quant(src->tok_emb, w->q_emb, lay.t[q8::T_EMB].values());
    quant(src->wq, w->q_wq, lay.t[q8::T_WQ].values());
    quant(src->wk, w->q_wk, lay.t[q8::T_WK].values());
    quant(src->wv, w->q_wv, lay.t[q8::T_WV].values());
    quant(src->wo, w->q_wo, lay.t[q8::T_WO].values());
    quant(src->w1, w->q_w13, 2 * lay.t[q8::T_W1].values());
    quant(src->w2, w->q_w2, lay.t[q8::T_W2].values());
    if (lay.t[q8::T_CLS].present) quant(src->wcls, w->q_cls, lay.t[q8::T_CLS].values());
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        set_error("l2z_weights_init_q8_from: quantization failed: %s", hipGetErrorString(e));
        l2z_weights_free(w);
        return L2Z_ERR_HIP;
    }
    *out = w;
    return L2Z_OK;
}

extern "C" int l2z_weights_q8_read(const l2z_weights *w, const char *tensor_name, int layer, int8_t *out_q, float *out_s)
{
    L2Z_CHECK(w != nullptr && tensor_name != nullptr && out_q != nullptr && out_s != nullptr, L2Z_ERR_INVALID,
              "l2z_weights_q8_read: null argument");
    L2Z_CHECK(w->is_q8(), L2Z_ERR_INVALID, "l2z_weights_q8_read: not int8 group-quantized weights");
    q8::Layout lay;
    L2Z_TRY(q8_layout_of("l2z_weights_q8_read", &w->cfg, w->shared, w->q8_gs, 0, false, &lay));
    const int t = q8::tensor_by_name(tensor_name);
    L2Z_CHECK(t >= 0, L2Z_ERR_INVALID, "l2z_weights_q8_read: no quantized tensor \"%s\"", tensor_name);
    const q8::Mat &m = lay.t[t];   // (wcls of a shared file: the embedding table's shape, served from it)
    L2Z_CHECK(layer >= 0 && (uint64_t)layer < m.layers, L2Z_ERR_INVALID, "l2z_weights_q8_read: layer %d of %s", layer, tensor_name);
    L2Z_HIP(hipSetDevice(w->device));
    L2Z_HIP(q8_copy_tensor(w, m, t, (size_t)layer, 1, out_q, out_s, false));
    return L2Z_OK;
}
