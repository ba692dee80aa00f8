// weights.cpp -- shard geometry, the llama2.c-v0 tensor table (main.zig:85-112) and the device
// resident Weights object of the C ABI (include/llama2_hip.h).
//
// Product code.  No CPU fallback anywhere: without a HIP device every compute entry point returns
// L2Z_ERR_NO_DEVICE.  Nothing under oracle/ is referenced.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "l2z_state.h"
#include "packed_w.h"
#include "q8_layout.h"
#include "tunables.h"

namespace l2z {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int make_shard(const l2z_config &c, const l2z_comm *comm, Shard *out)
{
    Shard s;
    s.rank = comm ? comm->rank : 0;
    s.world = comm ? comm->world : 1;
    L2Z_CHECK(c.dim > 0 && c.hidden_dim > 0 && c.n_layers > 0 && c.n_heads > 0 &&
                  c.n_kv_heads > 0 && c.vocab_size > 0 && c.seq_len > 0,
              L2Z_ERR_INVALID, "config: all seven fields must be positive");
    L2Z_CHECK(c.dim % c.n_heads == 0, L2Z_ERR_INVALID, "config: dim %% n_heads != 0");
    L2Z_CHECK(c.n_heads % c.n_kv_heads == 0, L2Z_ERR_INVALID, "config: n_heads %% n_kv_heads != 0");
    s.hs = c.dim / c.n_heads;
    L2Z_CHECK(s.hs % 2 == 0, L2Z_ERR_INVALID, "config: head_size must be even (RoPE pairs)");
    const int kv_dim = (int)(((int64_t)c.dim * c.n_kv_heads) / c.n_heads);
    int64_t a, b;
    L2Z_TRY(l2z_shard_range(c.dim, s.hs, s.rank, s.world, &a, &b));
    s.dim0 = (int)a;
    s.dim_loc = (int)(b - a);
    s.heads_loc = s.dim_loc / s.hs;
    L2Z_TRY(l2z_shard_range(kv_dim, s.hs, s.rank, s.world, &a, &b));
    s.kvd_loc = (int)(b - a);
    L2Z_TRY(l2z_shard_range(c.hidden_dim, 1, s.rank, s.world, &a, &b));
    s.hid0 = (int)a;
    s.hid_loc = (int)(b - a);
    L2Z_TRY(l2z_shard_range(c.vocab_size, 1, s.rank, s.world, &a, &b));
    s.v0 = (int)a;
    s.v_loc = (int)(b - a);
    // (a 1-rank RCCL communicator takes it too: the ncclAllReduce call path, testable on one GPU)
    s.scheme_b = tunables().scheme_b != 0 && comm != nullptr && (s.world > 1 || comm->nccl != nullptr);
    s.dimc_pad = pad_cols(s.dim_loc);
    s.hidc_pad = pad_cols(s.hid_loc);
    *out = s;
    return L2Z_OK;
}

int pad_cols(int n)
{
    const int n4 = (n + 3) / 4;
    return n > 768 ? ((n4 + 63) / 64) * 256 : n4 * 4;
}

std::vector<TensorDesc> tensor_table(const l2z_config &c, bool shared)
{
    const size_t V = c.vocab_size, dim = c.dim, hid = c.hidden_dim, L = c.n_layers;
    const size_t S = c.seq_len, hs = dim / c.n_heads, kvd = (dim * c.n_kv_heads) / c.n_heads;
    const float s_dim = sqrtf(3.0f / (float)dim), s_hid = sqrtf(3.0f / (float)hid);
    const float s_emb = 2.0f * s_dim;
    std::vector<TensorDesc> t = {
        {"token_embedding_table", 0, 1, V, dim, REPL, s_emb, 0.0f},   // :86
        {"rms_att_weight", 0, L, 1, dim, REPL, 0.1f, 1.0f},           // :88
        {"wq", 0, L, dim, dim, BY_Q_HEADS, s_dim, 0.0f},              // :90
        {"wk", 0, L, kvd, dim, BY_KV_HEADS, s_dim, 0.0f},             // :92
        {"wv", 0, L, kvd, dim, BY_KV_HEADS, s_dim, 0.0f},             // :94
        {"wo", 0, L, dim, dim, BY_DIM_ROWS, s_dim, 0.0f},             // :96
        {"rms_ffn_weight", 0, L, 1, dim, REPL, 0.1f, 1.0f},           // :98
        {"w1", 0, L, hid, dim, BY_HIDDEN, s_dim, 0.0f},               // :100
        {"w2", 0, L, dim, hid, BY_DIM_ROWS, s_hid, 0.0f},             // :102
        {"w3", 0, L, hid, dim, BY_HIDDEN, s_dim, 0.0f},               // :104
        {"rms_final_weight", 0, 1, 1, dim, REPL, 0.1f, 1.0f},         // :106
        {"freq_cis_real", 0, 1, 1, S * hs / 2, SKIP, 1.0f, 0.0f},     // :108 (never read)
        {"freq_cis_imag", 0, 1, 1, S * hs / 2, SKIP, 1.0f, 0.0f},     // :110
    };
    if (!shared) t.push_back({"wcls", 0, 1, V, dim, BY_VOCAB, s_emb, 0.0f});  // :112
    size_t off = 0;
    for (auto &d : t) {
        d.offset = off;
        off += d.count();
    }
    return t;
}

void shard_rows(const TensorDesc &d, const Shard &s, size_t *r0, size_t *r1)
{
    switch (d.kind) {
        case BY_Q_HEADS:
        case BY_DIM_ROWS: *r0 = s.dim0; *r1 = (size_t)s.dim0 + s.dim_loc; break;
        case BY_KV_HEADS: *r0 = (size_t)s.rank * s.kvd_loc; *r1 = *r0 + s.kvd_loc; break;
        case BY_HIDDEN: *r0 = s.hid0; *r1 = (size_t)s.hid0 + s.hid_loc; break;
        case BY_VOCAB: *r0 = s.v0; *r1 = (size_t)s.v0 + s.v_loc; break;
        default: *r0 = 0; *r1 = d.rows; break;
    }
}

int g_cus = 0;

int ensure_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device available (%s); this library has no CPU fallback",
                  e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        return L2Z_ERR_NO_DEVICE;
    }
    L2Z_CHECK(device >= 0 && device < n, L2Z_ERR_NO_DEVICE, "device %d out of range (%d present)",
              device, n);
    L2Z_HIP(hipSetDevice(device));
    if (g_cus == 0) {
        hipDeviceProp_t p;
        L2Z_HIP(hipGetDeviceProperties(&p, device));
        g_cus = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
    }
    return L2Z_OK;
}

int current_device_for(const l2z_comm *comm)
{
    if (comm) return comm->device;
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) d = 0;
    return d;
}

}  // namespace l2z

using namespace l2z;

namespace {

constexpr size_t kBlobSlackFloats = 1024;
bool is_w1(const TensorDesc &d) { return strcmp(d.name, "w1") == 0; }
bool is_w3(const TensorDesc &d) { return strcmp(d.name, "w3") == 0; }

// scheme B: Wo / W2 live here as this rank's COLUMNS of every row, each row padded with zeros to cpad floats
bool col_shard(const l2z_weights *w, const TensorDesc &d, size_t *c0, size_t *cl, size_t *cpad)
{
    if (!w->sh.scheme_b || d.kind != BY_DIM_ROWS) return false;
    const bool is_wo = strcmp(d.name, "wo") == 0;
    *c0 = is_wo ? w->sh.dim0 : w->sh.hid0;
    *cl = is_wo ? w->sh.dim_loc : w->sh.hid_loc;
    *cpad = is_wo ? w->sh.dimc_pad : w->sh.hidc_pad;
    return true;
}

// floats a tensor takes in the device blob: this rank's rows; W1's slot also holds W3's rows (interleaved),
// W3 has none of its own; the never-read freq_cis tables stay resident only in the unsharded layout (weights_read)
size_t slot_floats(const l2z_weights *w, const TensorDesc &d)
{
    size_t r0, r1;
    shard_rows(d, w->sh, &r0, &r1);
    if (d.kind == SKIP && !w->file_layout) return 0;
    if (is_w3(d)) return 0;
    size_t c0, cl, cpad;
    if (col_shard(w, d, &c0, &cl, &cpad)) return d.layers * d.rows * cpad;
    return d.layers * (r1 - r0) * d.cols * (is_w1(d) ? 2 : 1);
}

void carve_local(l2z_weights *w, const std::vector<TensorDesc> &tt)
{
    // device layout: the file's tensor order, each tensor (layers, rows_loc, cols); W1 | W3 row-interleaved in W1's slot
    size_t off = 0, off_w1 = 0;
    const float *base = w->blob;
    w->dev_off.assign(tt.size(), 0);
    for (size_t i = 0; i < tt.size(); i++) {
        const auto &d = tt[i];
        if (is_w1(d)) off_w1 = off;
        w->dev_off[i] = is_w3(d) ? off_w1 + d.cols : off;
        const float *p = base + w->dev_off[i];
        const std::string n = d.name;
        if (n == "token_embedding_table") w->tok_emb = p;
        else if (n == "rms_att_weight") w->rms_att = p;
        else if (n == "wq") w->wq = p;
        else if (n == "wk") w->wk = p;
        else if (n == "wv") w->wv = p;
        else if (n == "wo") w->wo = p;
        else if (n == "rms_ffn_weight") w->rms_ffn = p;
        else if (n == "w1") w->w1 = p;
        else if (n == "w2") w->w2 = p;
        else if (n == "w3") w->w3 = p;
        else if (n == "rms_final_weight") w->rms_final = p;
        else if (n == "wcls") w->wcls = p;
        off += slot_floats(w, d);
    }
    if (w->shared) w->wcls = w->tok_emb + (size_t)w->sh.v0 * w->cfg.dim;  // main.zig:112
}

size_t local_floats(const l2z_weights *w, const std::vector<TensorDesc> &tt)
{
    size_t off = 0;
    for (const auto &d : tt) off += slot_floats(w, d);
    return off;
}

// Host -> device copy of weight rows (main.zig:936-967 reads the whole file into the heap first; here
// the source is the caller's buffer, typically the mmapped checkpoint).  A plain hipMemcpy from the
// pageable mapping: the runtime stages it through its own pinned buffers at 54-56 GB/s for the
// 27 GB llama2-7b file (profiles/r02_upload_rate.txt).  An explicit pinned double buffer filled by
// eight host threads was measured beside it and was no faster (46-53 GB/s), so it is not kept.
hipError_t upload(float *dst, const float *src, size_t n_floats)
{
    const size_t piece = (size_t)256 << 20;  // floats: 1 GiB per call
    hipError_t e = hipSuccess;
    for (size_t o = 0; o < n_floats && e == hipSuccess; o += piece) {
        const size_t n = n_floats - o < piece ? n_floats - o : piece;
        e = hipMemcpy(dst + o, src + o, n * sizeof(float), hipMemcpyHostToDevice);
    }
    return e;
}

int weights_alloc(const l2z_config *config, int shared_weights, const l2z_comm *comm,
                  l2z_weights **out, std::vector<TensorDesc> *tt_out)
{
    L2Z_CHECK(config != nullptr && out != nullptr, L2Z_ERR_INVALID, "weights_init: null argument");
    const int dev = current_device_for(comm);
    L2Z_TRY(ensure_device(dev));
    Shard sh;
    L2Z_TRY(make_shard(*config, comm, &sh));
    static std::atomic<uint64_t> next_uid{1};
    l2z_weights *w = new l2z_weights();
    w->uid = next_uid.fetch_add(1);
    w->cfg = *config;
    w->shared = shared_weights ? 1 : 0;
    w->device = dev;
    w->sh = sh;
    w->file_layout = sh.world == 1 && !sh.scheme_b;
    *tt_out = tensor_table(*config, w->shared != 0);
    w->blob_floats = local_floats(w, *tt_out);
    // + a zeroed slack: the batched prefill's GEMMs multiply whole stages of K and read up to 3 x 256 floats past the
    // end of a W row against zero activation columns (prefill_common.h pad_k); past the LAST row of the LAST tensor
    // that is here (everywhere else it is the next row or the next tensor: finite)
    hipError_t e = hipMalloc(&w->blob, (w->blob_floats + kBlobSlackFloats) * sizeof(float));
    if (e == hipSuccess) e = hipMemset(w->blob + w->blob_floats, 0, kBlobSlackFloats * sizeof(float));
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) for weights failed: %s", w->blob_floats * sizeof(float),
                  hipGetErrorString(e));
        delete w;
        return e == hipErrorOutOfMemory ? L2Z_ERR_OOM : L2Z_ERR_HIP;
    }
    carve_local(w, *tt_out);
    *out = w;
    return L2Z_OK;
}

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

// ... of every kind of row launch of the decode, in the order of what each saves per token (a device short of memory
// keeps the kinds that pay most).  Unsharded weights of widths the row kernel runs only; everything else (prefill, the
// batched / wide / verify families, shards, l2z_weights_read, the embedding-row lookup) keeps reading the f32 blob.
void build_packed(l2z_weights *w)
{
    if (tunables().packed_w == 0 || !w->file_layout) return;
    const l2z_config &c = w->cfg;
    const size_t dim = c.dim, hid = c.hidden_dim, kvd = (size_t)c.dim / c.n_heads * c.n_kv_heads;
    const int L = c.n_layers;
    using Slots = std::vector<l2z_weights::PkMat>;
    const auto mat = [](const float *src, size_t rows, size_t cols) {
        l2z_weights::PkMat m;
        m.src = src; m.rows = (int)rows; m.cols = (int)cols;
        return m;
    };
    if (pk::width_ok(c.dim)) {
        Slots s13, sqkv, so, scls;
        for (int l = 0; l < L; l++) {
            s13.push_back(mat(w->w1 + (size_t)l * hid * 2 * dim, 2 * hid, dim));
            sqkv.push_back(mat(w->wq + (size_t)l * dim * dim, dim, dim));
            sqkv.push_back(mat(w->wk + (size_t)l * kvd * dim, kvd, dim));
            sqkv.push_back(mat(w->wv + (size_t)l * kvd * dim, kvd, dim));
            so.push_back(mat(w->wo + (size_t)l * dim * dim, dim, dim));
        }
        scls.push_back(mat(w->wcls, c.vocab_size, dim));  // shared embeddings: a copy of the embedding table
        build_packed_kind(w, KIND_FFN13, 1, std::move(s13));
        build_packed_kind(w, KIND_QKV, 3, std::move(sqkv));
        build_packed_kind(w, KIND_WO, 1, std::move(so));
        build_packed_kind(w, KIND_CLS, 1, std::move(scls));
    }
    if (pk::width_ok(c.hidden_dim)) {
        Slots s2;
        for (int l = 0; l < L; l++) s2.push_back(mat(w->w2 + (size_t)l * dim * hid, dim, hid));
        build_packed_kind(w, KIND_FFN2, 1, std::move(s2));
    }
}

}  // namespace

extern "C" int l2z_abi_version(void) { return L2Z_ABI_VERSION; }
extern "C" const char *l2z_last_error(void) { return l2z::g_err; }

extern "C" int l2z_device_count(int *out_n)
{
    L2Z_CHECK(out_n != nullptr, L2Z_ERR_INVALID, "l2z_device_count: null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *out_n = n;
    return L2Z_OK;
}

extern "C" int l2z_device_info(int dev, char *name, size_t cap, int *out_cus, uint64_t *out_hbm)
{
    L2Z_TRY(ensure_device(dev));
    hipDeviceProp_t p;
    L2Z_HIP(hipGetDeviceProperties(&p, dev));
    // some boxes report an empty marketing name
    if (name && cap) snprintf(name, cap, "%s (%s)", p.name[0] ? p.name : "AMD GPU", p.gcnArchName);
    if (out_cus) *out_cus = p.multiProcessorCount;
    if (out_hbm) *out_hbm = (uint64_t)p.totalGlobalMem;
    return L2Z_OK;
}

// src/main.zig:73 Weights.init
extern "C" int l2z_weights_init(const l2z_config *config, const float *data, size_t n_floats,
                                int shared_weights, const l2z_comm *comm, l2z_weights **out)
{
    L2Z_CHECK(data != nullptr, L2Z_ERR_INVALID, "l2z_weights_init: null data");
    std::vector<TensorDesc> tt;
    l2z_weights *w = nullptr;
    L2Z_TRY(weights_alloc(config, shared_weights, comm, &w, &tt));
    const size_t need = tt.back().offset + tt.back().count();
    if (n_floats < need) {
        set_error("l2z_weights_init: blob has %zu f32, config needs %zu", n_floats, need);
        l2z_weights_free(w);
        return L2Z_ERR_INVALID;
    }
    // this rank's rows of every tensor, straight from the caller's buffer (typically the mmapped checkpoint);
    // W1 / W3 rows go through a device staging buffer of one layer and are spread over the shared slot there
    hipError_t e = hipSuccess;
    float *stage = nullptr;
    for (size_t i = 0; i < tt.size() && e == hipSuccess; i++) {
        const auto &d = tt[i];
        if (d.kind == SKIP && !w->file_layout) continue;
        size_t r0, r1;
        shard_rows(d, w->sh, &r0, &r1);
        const size_t rl = r1 - r0;
        float *dst = w->blob + w->dev_off[i];
        size_t c0, cl, cpad;
        if (col_shard(w, d, &c0, &cl, &cpad)) {
            // columns [c0, c0 + cl) of every row; the pad columns stay zero
            e = hipMemset(dst, 0, d.layers * d.rows * cpad * sizeof(float));
            for (size_t l = 0; l < d.layers && e == hipSuccess; l++)
                e = hipMemcpy2D(dst + l * d.rows * cpad, cpad * sizeof(float), data + d.offset + l * d.rows * d.cols + c0,
                                d.cols * sizeof(float), cl * sizeof(float), d.rows, hipMemcpyHostToDevice);
            continue;
        }
        if (is_w1(d) || is_w3(d)) {
            // in pieces of <= 64 MB through TWO staging buffers: a whole layer (180 MB at the 7B shape, ~1 GB at wider
            // ones) allocated after the blob could be the allocation that no longer fits, and a device-wide
            // synchronise per layer serialised the load.  A staging buffer is written again two pieces later; the
            // host-to-device copy and the spreading kernel both run in the null stream, in order.
            const size_t piece_rows = std::max<size_t>(1, std::min<size_t>(rl, ((size_t)64 << 20) / (d.cols * sizeof(float))));
            if (stage == nullptr) e = hipMalloc((void **)&stage, 2 * piece_rows * d.cols * sizeof(float));
            size_t n_piece = 0;
            for (size_t l = 0; l < d.layers && e == hipSuccess; l++) {
                for (size_t r = 0; r < rl && e == hipSuccess; r += piece_rows, n_piece++) {
                    const size_t nr = std::min(piece_rows, rl - r);
                    float *sb = stage + (n_piece & 1) * piece_rows * d.cols;
                    e = upload(sb, data + d.offset + (l * d.rows + r0 + r) * d.cols, nr * d.cols);
                    if (e == hipSuccess) e = launch_copy_rows(dst + (l * rl + r) * 2 * d.cols, 2 * d.cols, sb, nr, d.cols, nullptr);
                }
            }
            if (e == hipSuccess) e = hipDeviceSynchronize();
        } else if (rl == d.rows) {
            e = upload(dst, data + d.offset, d.count());
        } else {
            for (size_t l = 0; l < d.layers && e == hipSuccess; l++)
                e = upload(dst + l * rl * d.cols, data + d.offset + (l * d.rows + r0) * d.cols, rl * d.cols);
        }
    }
    if (stage) (void)hipFree(stage);
    if (e != hipSuccess) {
        set_error("weight upload failed: %s", hipGetErrorString(e));
        l2z_weights_free(w);
        return L2Z_ERR_HIP;
    }
    build_packed(w);
    *out = w;
    return L2Z_OK;
}

extern "C" int l2z_weights_init_synthetic(const l2z_config *config, int shared_weights,
                                          uint64_t seed, const l2z_comm *comm, l2z_weights **out)
{
    std::vector<TensorDesc> tt;
    l2z_weights *w = nullptr;
    L2Z_TRY(weights_alloc(config, shared_weights, comm, &w, &tt));
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < tt.size(); i++) {
        const auto &d = tt[i];
        if (d.kind == SKIP && !w->file_layout) continue;
        size_t r0, r1;
        shard_rows(d, w->sh, &r0, &r1);
        const size_t rl = r1 - r0;
        const bool pair = is_w1(d) || is_w3(d);  // rows 2 * cols apart in the shared slot
        size_t c0, cl, cpad;
        if (col_shard(w, d, &c0, &cl, &cpad)) {
            float *dst = w->blob + w->dev_off[i];
            e = hipMemsetAsync(dst, 0, d.layers * d.rows * cpad * sizeof(float), nullptr);
            for (size_t l = 0; l < d.layers && e == hipSuccess; l++)
                e = launch_synth_fill(dst + l * d.rows * cpad, d.offset + l * d.rows * d.cols + c0, d.rows * cl, seed, d.scale, d.bias,
                                      nullptr, cl, cpad, d.cols);
            continue;
        }
        for (size_t l = 0; l < d.layers && e == hipSuccess; l++) {
            const uint64_t base = d.offset + (l * d.rows + r0) * d.cols;
            e = launch_synth_fill(w->blob + w->dev_off[i] + l * rl * d.cols * (pair ? 2 : 1), base, rl * d.cols, seed, d.scale,
                                  d.bias, nullptr, pair ? d.cols : 0, pair ? 2 * d.cols : 0);
        }
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        set_error("synthetic weight fill failed: %s", hipGetErrorString(e));
        l2z_weights_free(w);
        return L2Z_ERR_HIP;
    }
    build_packed(w);
    *out = w;
    return L2Z_OK;
}

// offset / count address the FILE's order (main.zig:85-112); the device blob differs from it in W1 / W3 (rows
// interleaved in one slot), so the range is served tensor by tensor and, there, row by row
extern "C" int l2z_weights_read(const l2z_weights *w, size_t offset, size_t count, float *out)
{
    L2Z_CHECK(w != nullptr && out != nullptr, L2Z_ERR_INVALID, "l2z_weights_read: null argument");
    L2Z_CHECK(!w->is_q8(), L2Z_ERR_INVALID, "l2z_weights_read: int8 group-quantized weights hold no f32 tensors (l2z_weights_q8_read)");
    L2Z_CHECK(w->file_layout, L2Z_ERR_INVALID, "l2z_weights_read: only for unsharded weights");
    L2Z_CHECK(offset + count <= w->blob_floats, L2Z_ERR_INVALID, "l2z_weights_read: out of range");
    L2Z_HIP(hipSetDevice(w->device));
    const std::vector<TensorDesc> tt = tensor_table(w->cfg, w->shared != 0);
    const size_t lo = offset, hi = offset + count;
    for (size_t i = 0; i < tt.size(); i++) {
        const auto &d = tt[i];
        const size_t t0 = std::max(lo, d.offset), t1 = std::min(hi, d.offset + d.count());
        if (t0 >= t1) continue;
        if (!(is_w1(d) || is_w3(d))) {
            L2Z_HIP(hipMemcpy(out + (t0 - lo), w->blob + w->dev_off[i] + (t0 - d.offset), (t1 - t0) * sizeof(float),
                              hipMemcpyDeviceToHost));
            continue;
        }
        for (size_t f = t0; f < t1;) {  // row r of the tensor sits 2 * cols * r into the slot
            const size_t r = (f - d.offset) / d.cols, c = (f - d.offset) % d.cols;
            const float *src = w->blob + w->dev_off[i] + r * 2 * d.cols + c;
            const size_t whole = c == 0 ? (t1 - f) / d.cols : 0;  // whole rows from here: one strided copy
            if (whole > 0) {
                L2Z_HIP(hipMemcpy2D(out + (f - lo), d.cols * sizeof(float), src, 2 * d.cols * sizeof(float),
                                    d.cols * sizeof(float), whole, hipMemcpyDeviceToHost));
                f += whole * d.cols;
            } else {  // a partial row at either end of the range
                const size_t n = std::min(d.cols - c, t1 - f);
                L2Z_HIP(hipMemcpy(out + (f - lo), src, n * sizeof(float), hipMemcpyDeviceToHost));
                f += n;
            }
        }
    }
    return L2Z_OK;
}

extern "C" void l2z_weights_free(l2z_weights *w)
{
    if (!w) return;
    if (w->blob) (void)hipFree(w->blob);
    if (w->q8_blob) (void)hipFree(w->q8_blob);
    for (auto &k : w->pk)
        if (k.blob) (void)hipFree(k.blob);
    delete w;
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
