// kind_rows.h -- which weights a row launch of the decode pass reads: for (weights, shard, kind, layer) the launch's one
// to three segments, each with its f32 rows, its shape and -- where the object holds them -- its packed slot (DESIGN.md
// 4.9) and its int8 values and scales; and how a launch's argument block takes them.  Computed on
// demand, nothing is kept in l2z_weights.  The packed-copy builder (weights_packed.cpp) lists its slots from it and the
// layer walk (forward.cpp) attaches from it: the segment order (q, k, v) is this file's alone.
#pragma once
#include "l2z_state.h"

namespace l2z {

struct KindSeg {
    const float *f32;                  // row 0 of the layer's matrix (null: the object has no f32 matrix)
    int rows, cols;                    // ffn13: the 2 * hid_loc rows of the W1 | W3 interleaved slot
    const l2z_weights::PkMat *pk;      // the packed slot, null: none
    const int8_t *q;                   // int8 weights: values [rows][cols] and scales [rows][cols / gs]; else null
    const float *qs;
};
struct KindRows {
    int n;   // segments
    KindSeg seg[kMaxSeg];
};

// Rows are this rank's (sh); under scheme B Wo and W2 are its COLUMNS of every row, padded (Shard::dimc_pad / hidc_pad)
inline KindRows kind_rows(const l2z_weights *w, const Shard &sh, int kind, int layer)
{
    const l2z_config &c = w->cfg;
    KindRows r = {};
    const auto add = [&](const float *f32, const l2z_weights::Q8Mat &qm, int rows, int cols) {
        KindSeg &g = r.seg[r.n];
        const size_t at = (size_t)layer * rows * cols;
        g.rows = rows;
        g.cols = cols;
        if (f32 != nullptr) g.f32 = f32 + at;
        g.pk = w->pk_slot(kind, layer, r.n);
        if (w->is_q8()) {
            g.q = qm.q + at;
            g.qs = qm.s + at / (size_t)w->q8_gs;
        }
        r.n++;
    };
    switch (kind) {
        case KIND_QKV:
            add(w->wq, w->q_wq, sh.dim_loc, c.dim);
            add(w->wk, w->q_wk, sh.kvd_loc, c.dim);
            add(w->wv, w->q_wv, sh.kvd_loc, c.dim);
            break;
        case KIND_WO:
            if (sh.scheme_b) add(w->wo, w->q_wo, c.dim, sh.dimc_pad);
            else add(w->wo, w->q_wo, sh.dim_loc, c.dim);
            break;
        case KIND_FFN13: add(w->w1, w->q_w13, 2 * sh.hid_loc, c.dim); break;
        case KIND_FFN2:
            if (sh.scheme_b) add(w->w2, w->q_w2, c.dim, sh.hidc_pad);
            else add(w->w2, w->q_w2, sh.dim_loc, c.hidden_dim);
            break;
        case KIND_CLS: add(w->wcls, w->q_cls, sh.v_loc, c.dim); break;   // (one per model: layer 0)
        default: break;
    }
    return r;
}

// The f32 launch takes the segments' rows and, with `packed`, their packed slots: every segment's or none (a launch
// streams one form), each slot with its own base exponent and -- the 28-bit form -- its patch records.  ffn13: w1 is W3's
// row 0, one row into the interleaved slot (the kernels derive it from w0)
inline void attach_rows(MatvecArgs &a, const KindRows &r, int kind, bool packed)
{
    const float **wf[kMaxSeg] = {&a.w0, &a.w1, &a.w2};
    const uint32_t **pk[kMaxSeg] = {&a.pk, &a.pk1, &a.pk2}, **rec[kMaxSeg] = {&a.pk_rec, &a.pk_rec1, &a.pk_rec2};
    int *pk_e[kMaxSeg] = {&a.pk_e, &a.pk_e1, &a.pk_e2};
    for (int j = 0; j < r.n; j++) {
        *wf[j] = r.seg[j].f32;
        packed = packed && r.seg[j].pk != nullptr;
    }
    if (kind == KIND_FFN13) a.w1 = a.w0 + r.seg[0].cols;
    for (int j = 0; j < r.n && packed; j++) {
        *pk[j] = r.seg[j].pk->p;
        *pk_e[j] = r.seg[j].pk->e;
        *rec[j] = r.seg[j].pk->rec;
    }
}

// ... and the int8 launch their values and scales
inline void attach_rows(Q8MatvecArgs &a, const KindRows &r)
{
    const int8_t **q[kMaxSeg] = {&a.q0, &a.q1, &a.q2};
    const float **qs[kMaxSeg] = {&a.s0, &a.s1, &a.s2};
    for (int j = 0; j < r.n; j++) {
        *q[j] = r.seg[j].q;
        *qs[j] = r.seg[j].qs;
    }
}

}  // namespace l2z
