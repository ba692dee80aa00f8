// weights_packed.cpp -- the packed copy of the decode's row mat-vec weights (packed_w.h): its builder, run
// by the f32 weights' init calls (weights.cpp), and the l2z_weights_packed_* read-back ABI (include/llama2_hip_test.h).
#include <cstdlib>
#include <cstring>

#include "kind_rows.h"
#include "l2z_state.h"
#include "packed_w.h"
#include "tunables.h"

using namespace l2z;

namespace {

// The packed copy of one kind's slots (packed_w.h), built on the device from the complete f32 blob: a
// stats pass per slot, one host read of the stats, an escape count of the 28-bit candidates and one host read of it, one
// allocation for the kind, a packing pass per encodable slot in the form picked for it.  A
// slot with an odd number of rows has no pairs to pack and stays f32 like one outside the format.  Best effort: a failed
// allocation or launch leaves this kind without a copy (f32 decode), never failing init.
void build_packed_kind(l2z_weights *w, int kind, int per_layer, std::vector<l2z_weights::PkMat> slots)
{
    l2z_weights::PkKind &k = w->pk[kind];
    k.per_layer = per_layer;
    k.slots = std::move(slots);
    const size_t n = k.slots.size();
    std::vector<uint32_t> stats(3 * n);
    for (size_t i = 0; i < n; i++) {
        stats[3 * i] = 0;
        stats[3 * i + 1] = 255;
        stats[3 * i + 2] = 0;
    }
    uint32_t *d_stats = nullptr;
    hipError_t e = hipMalloc((void **)&d_stats, stats.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d_stats, stats.data(), stats.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    for (size_t i = 0; i < n && e == hipSuccess; i++)
        e = launch_pk_stats(k.slots[i].src, (size_t)k.slots[i].rows * k.slots[i].cols, d_stats + 3 * i, nullptr);
    if (e == hipSuccess) e = hipMemcpy(stats.data(), d_stats, stats.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    const auto fits = [&](size_t i) {
        return k.slots[i].rows % 2 == 0 && pk::encodable(stats[3 * i], stats[3 * i + 1], stats[3 * i + 2]);
    };
    // the 28-bit form (pk28) for the slots of one-batch rows: one more pass counts each pair's escapes, one word a slot
    // comes back (the most any of its pairs has) and a slot within the record's eight entries takes it.  q | k | v streams
    // one form per launch: a layer whose three slots do not all take 28 bits keeps 29 in all three
    std::vector<int> bits(n, 29);
    const Tunables &tn = tunables();
    const auto cand28 = [&](size_t i) {
        return tn.packed_bits == 28 && ((tn.packed28_kinds >> kind) & 1) && fits(i) && pk28::width_ok(k.slots[i].cols);
    };
    std::vector<uint32_t> esc(n, 0);
    bool any28 = false;
    for (size_t i = 0; i < n; i++) any28 = any28 || cand28(i);
    if (e == hipSuccess && any28) {
        e = hipMemset(d_stats, 0, n * sizeof(uint32_t));  // (3 n words: room for one a slot)
        for (size_t i = 0; i < n && e == hipSuccess; i++)
            if (cand28(i)) e = launch_pk28_count(k.slots[i].src, k.slots[i].rows, k.slots[i].cols, (int)stats[3 * i], d_stats + i, nullptr);
        if (e == hipSuccess) e = hipMemcpy(esc.data(), d_stats, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
        for (size_t i = 0; i < n; i++)
            if (cand28(i) && esc[i] <= (uint32_t)pk28::kMaxEsc) bits[i] = 28;
        for (size_t i = 0; per_layer > 1 && i + per_layer <= n; i += per_layer) {
            bool all = true;
            for (int j = 0; j < per_layer; j++) all = all && bits[i + j] == 28;
            for (int j = 0; j < per_layer && !all; j++) bits[i + j] = 29;
        }
    }
    if (d_stats) (void)hipFree(d_stats);
    // a slot's dwords: its stream and, behind it, a 28-bit slot's records (both whole multiples of 64 bytes)
    const auto stream_dw = [&](size_t i) -> size_t {
        const auto &m = k.slots[i];
        if (!fits(i)) return 0;
        return (size_t)(m.rows / 2) * (bits[i] == 28 ? (size_t)pk28::kPairDw : pk::pair_dw(m.cols / 4));
    };
    const auto dwords = [&](size_t i) -> size_t {
        return stream_dw(i) + (stream_dw(i) && bits[i] == 28 ? (size_t)(k.slots[i].rows / 2) * pk28::kRecDw : 0);
    };
    size_t total = 0;
    for (size_t i = 0; i < n; i++) total += dwords(i);
    if (e == hipSuccess && total > 0) {
        e = hipMalloc((void **)&k.blob, total * sizeof(uint32_t));
        if (e != hipSuccess) k.blob = nullptr;  // no room for the copy: this kind streams the f32 weights
    }
    size_t off = 0;
    for (size_t i = 0; i < n && e == hipSuccess && k.blob; i++) {
        auto &m = k.slots[i];
        if (dwords(i) == 0) continue;
        if (bits[i] == 28) {
            uint32_t *rec = k.blob + off + stream_dw(i);
            e = launch_pk28_pack(m.src, m.rows, m.cols, (int)stats[3 * i], k.blob + off, rec, nullptr);
            m.rec = rec;
        } else {
            e = launch_pk_pack(m.src, m.rows, m.cols, (int)stats[3 * i], k.blob + off, nullptr);
        }
        m.p = k.blob + off;
        m.e = (int)stats[3 * i];
        k.packed++;
        off += dwords(i);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (k.blob) (void)hipFree(k.blob);
        k.blob = nullptr;
        for (auto &m : k.slots) m.p = m.rec = nullptr;
        k.packed = 0;
    }
}

}  // namespace

// ... of every kind of row launch of the decode, in the order of what each saves per token (a device short of memory
// keeps the kinds that pay most).  Unsharded weights of widths the row kernel runs only; everything else (prefill, the
// batched / wide / verify families, shards, l2z_weights_read, the embedding-row lookup) keeps reading the f32 blob.
// A kind's slots are the segments its launches read (kind_rows.h), layer by layer; the classifier's one slot is, with
// shared embeddings, a copy of the embedding table
void l2z::build_packed(l2z_weights *w)
{
    if (tunables().packed_w == 0 || !w->file_layout) return;
    for (int kind : {KIND_FFN13, KIND_QKV, KIND_WO, KIND_CLS, KIND_FFN2}) {
        std::vector<l2z_weights::PkMat> slots;
        int per_layer = 0;
        for (int l = 0; l < (kind == KIND_CLS ? 1 : w->cfg.n_layers); l++) {
            const KindRows r = kind_rows(w, w->sh, kind, l);
            per_layer = r.n;
            for (int j = 0; j < r.n; j++) {
                l2z_weights::PkMat m;
                m.src = r.seg[j].f32; m.rows = r.seg[j].rows; m.cols = r.seg[j].cols;
                slots.push_back(m);
            }
        }
        if (pk::width_ok(slots[0].cols)) build_packed_kind(w, kind, per_layer, std::move(slots));
    }
}

namespace {

int packed_read_slot(const l2z_weights *w, int kind, int layer, int j, float *out, size_t n_floats)
{
    const l2z_weights::PkKind &k = w->pk[kind];
    L2Z_CHECK(layer >= 0 && j >= 0 && j < k.per_layer && (size_t)layer * k.per_layer + j < k.slots.size(), L2Z_ERR_INVALID,
              "l2z_weights_packed_read: no packed slot %d of layer %d of kind %s", j, layer, kKindNames[kind]);
    const l2z_weights::PkMat *pm = w->pk_slot(kind, layer, j);
    L2Z_CHECK(pm != nullptr, L2Z_ERR_STATE, "l2z_weights_packed_read: slot %d of layer %d of kind %s is not packed", j, layer,
              kKindNames[kind]);
    const size_t count = (size_t)pm->rows * pm->cols;
    L2Z_CHECK(n_floats >= count, L2Z_ERR_INVALID, "l2z_weights_packed_read: need %zu floats", count);
    L2Z_HIP(hipSetDevice(w->device));
    float *d = nullptr;
    L2Z_HIP(hipMalloc((void **)&d, count * sizeof(float)));
    hipError_t e = pm->rec != nullptr ? launch_pk28_unpack(pm->p, pm->rec, pm->rows, pm->cols, pm->e, d, nullptr)
                                      : launch_pk_unpack(pm->p, pm->rows, pm->cols, pm->e, d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d, count * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    L2Z_HIP(e);
    return L2Z_OK;
}

}  // namespace

extern "C" int l2z_weights_packed_count(const l2z_weights *w, int *n_packed, int *n_candidates)
{
    return l2z_weights_packed_count_kind(w, KIND_FFN13, n_packed, n_candidates);
}

extern "C" int l2z_weights_packed_read(const l2z_weights *w, int layer, float *out, size_t n_floats)
{
    L2Z_CHECK(w != nullptr && out != nullptr, L2Z_ERR_INVALID, "l2z_weights_packed_read: null argument");
    return packed_read_slot(w, KIND_FFN13, layer, 0, out, n_floats);
}

extern "C" int l2z_weights_packed_count_kind(const l2z_weights *w, int kind, int *n_packed, int *n_candidates)
{
    L2Z_CHECK(w != nullptr && n_packed != nullptr && n_candidates != nullptr, L2Z_ERR_INVALID,
              "l2z_weights_packed_count: null argument");
    L2Z_CHECK(kind >= 0 && kind < KIND_COUNT, L2Z_ERR_INVALID, "l2z_weights_packed_count_kind: bad kind %d", kind);
    *n_packed = w->pk[kind].packed;
    *n_candidates = (int)w->pk[kind].slots.size();
    return L2Z_OK;
}

extern "C" int l2z_weights_packed_bits_kind(const l2z_weights *w, int kind, int layer, int slot, int *bits)
{
    L2Z_CHECK(w != nullptr && bits != nullptr, L2Z_ERR_INVALID, "l2z_weights_packed_bits_kind: null argument");
    L2Z_CHECK(kind >= 0 && kind < KIND_COUNT, L2Z_ERR_INVALID, "l2z_weights_packed_bits_kind: bad kind %d", kind);
    const l2z_weights::PkKind &k = w->pk[kind];
    L2Z_CHECK(layer >= 0 && slot >= 0 && slot < k.per_layer && (size_t)layer * k.per_layer + slot < k.slots.size(), L2Z_ERR_INVALID,
              "l2z_weights_packed_bits_kind: no slot %d of layer %d of kind %s", slot, layer, kKindNames[kind]);
    const l2z_weights::PkMat *pm = w->pk_slot(kind, layer, slot);
    *bits = pm != nullptr ? pm->bits() : 0;
    return L2Z_OK;
}

extern "C" int l2z_weights_packed_read_kind(const l2z_weights *w, int kind, int layer, int slot, float *out, size_t n_floats)
{
    L2Z_CHECK(w != nullptr && out != nullptr, L2Z_ERR_INVALID, "l2z_weights_packed_read: null argument");
    L2Z_CHECK(kind >= 0 && kind < KIND_COUNT, L2Z_ERR_INVALID, "l2z_weights_packed_read_kind: bad kind %d", kind);
    return packed_read_slot(w, kind, layer, slot, out, n_floats);
}
