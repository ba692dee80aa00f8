// q8_layout.h -- where every tensor of a llama2.c version-2 checkpoint body lies.  Plain C++: no HIP,
// nothing of the library, so tests/q8_layout_check.cpp runs it under the sanitizers on its own.
//
// The body is the file from byte 256 on: three f32 tensors (rms_att_weight [L, dim], rms_ffn_weight [L, dim],
// rms_final_weight [dim]), then the quantized tensors, each as its int8 values followed by its f32 scales (one per group
// of `gs` consecutive values): the token embedding, wq of every layer, then wk, wv, wo, w1, w2, w3 likewise, then wcls
// unless the classifier is the embedding table.
#pragma once
#include <cstddef>
#include <cstdint>

namespace l2z {
namespace q8 {

enum Tensor { T_EMB = 0, T_WQ, T_WK, T_WV, T_WO, T_W1, T_W2, T_W3, T_CLS, T_COUNT };
static const char *const kTensorNames[T_COUNT] = {"token_embedding_table", "wq", "wk", "wv", "wo", "w1", "w2", "w3", "wcls"};

enum Status { LAYOUT_OK = 0, BAD_GROUP_SIZE, BAD_DIMS, NOT_DIVISIBLE, BODY_TOO_SHORT };

inline const char *status_text(int st)
{
    switch (st) {
        case LAYOUT_OK: return "ok";
        case BAD_GROUP_SIZE: return "group_size must be 32 or 64";
        case BAD_DIMS: return "every dimension must be positive, dim a multiple of n_heads, n_heads of n_kv_heads";
        case NOT_DIVISIBLE: return "dim and hidden_dim must be multiples of group_size";
        default: return "the body is shorter than the config needs";
    }
}

struct Dims {
    int dim, hidden_dim, n_layers, n_heads, n_kv_heads, vocab_size, seq_len;
};

// one quantized tensor: `layers` matrices of rows x cols; layer l's values start at q_off + l * rows * cols bytes, its
// scales (f32, rows * cols / gs of them) at s_off + l * (rows * cols / gs) * 4
struct Mat {
    uint64_t q_off, s_off;
    uint64_t layers, rows, cols;
    bool present;
    uint64_t values() const { return layers * rows * cols; }
};

struct Layout {
    int gs;
    uint64_t rms_att_off, rms_ffn_off, rms_final_off;  // bytes; L * dim, L * dim, dim floats
    Mat t[T_COUNT];
    uint64_t total;  // bytes of the whole body
};

inline bool group_size_ok(int gs) { return gs == 32 || gs == 64; }

// the layout of a body, without looking at one
inline int layout(const Dims &c, bool shared_classifier, int gs, Layout *out)
{
    if (!group_size_ok(gs)) return BAD_GROUP_SIZE;
    if (c.dim <= 0 || c.hidden_dim <= 0 || c.n_layers <= 0 || c.n_heads <= 0 || c.n_kv_heads <= 0 || c.vocab_size <= 0 ||
        c.seq_len <= 0 || c.dim % c.n_heads != 0 || c.n_heads % c.n_kv_heads != 0)
        return BAD_DIMS;
    if (c.dim % gs != 0 || c.hidden_dim % gs != 0) return NOT_DIVISIBLE;
    const uint64_t dim = (uint64_t)c.dim, hid = (uint64_t)c.hidden_dim, L = (uint64_t)c.n_layers, V = (uint64_t)c.vocab_size;
    const uint64_t kvd = dim / (uint64_t)c.n_heads * (uint64_t)c.n_kv_heads;
    Layout o = {};
    o.gs = gs;
    uint64_t off = 0;
    o.rms_att_off = off; off += L * dim * 4;
    o.rms_ffn_off = off; off += L * dim * 4;
    o.rms_final_off = off; off += dim * 4;
    const uint64_t shape[T_COUNT][3] = {{1, V, dim},   {L, dim, dim}, {L, kvd, dim}, {L, kvd, dim}, {L, dim, dim},
                                        {L, hid, dim}, {L, dim, hid}, {L, hid, dim}, {1, V, dim}};
    for (int i = 0; i < T_COUNT; i++) {
        Mat &m = o.t[i];
        m.layers = shape[i][0]; m.rows = shape[i][1]; m.cols = shape[i][2];
        m.present = !(i == T_CLS && shared_classifier);
        if (!m.present) continue;
        m.q_off = off; off += m.values();
        m.s_off = off; off += m.values() / (uint64_t)gs * 4;
    }
    o.total = off;
    *out = o;
    return LAYOUT_OK;
}

// ... and against a body of n_bytes
inline int layout_checked(const Dims &c, bool shared_classifier, int gs, uint64_t n_bytes, Layout *out)
{
    const int st = layout(c, shared_classifier, gs, out);
    if (st != LAYOUT_OK) return st;
    return n_bytes < out->total ? BODY_TOO_SHORT : LAYOUT_OK;
}

inline int tensor_by_name(const char *name)
{
    if (name == nullptr) return -1;
    for (int i = 0; i < T_COUNT; i++) {
        const char *a = kTensorNames[i], *b = name;
        while (*a && *a == *b) a++, b++;
        if (*a == 0 && *b == 0) return i;
    }
    return -1;
}

}  // namespace q8
}  // namespace l2z
