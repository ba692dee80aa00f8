// batch_host.cpp -- host side of the batched decode step (l2z_transformer_batch, l2z_argmax_batch): up to
// L2Z_BATCH_MAX independent sequences advanced by one token with one sweep of the weights.  Kernels: the short-prompt
// GEMM forms with per-row epilogues (prefill_skinny.hip, G_*_ROWS) and batch_decode.hip.  Also what a batch of samples
// needs around the step: the on-device sampler l2z_sample_batch (sample_batch.hip) and the prompt copy
// l2z_runstate_fork.  And l2z_verify: the same step with the rows being consecutive positions of ONE sequence
// (speculative greedy decoding), attention and verdict by verify.hip.  And l2z_verify_batch: that pass for the rows of
// several sequences at once, attention and verdict per sequence by verify_batch.hip.  And l2z_verify_tree: the rows being
// the nodes of a tree of guesses on one sequence, attention, verdict and compaction by verify_tree.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "batch_decode.h"
#include "l2z_state.h"
#include "prefill_common.h"

static_assert(l2z::kBatchMax == L2Z_BATCH_MAX, "include/llama2_hip.h L2Z_BATCH_MAX");

namespace l2z {

// Scratch of the batched step, owned by the runstate that is states[0] of a call (allocated on its first such call,
// freed with it): the activation rows of kBatchMax sequences, the attention scores, the device table and its pinned
// host twin, and the events that order the pass against the runstates' own streams.
struct BatchScratch {
    float *x = nullptr, *xn = nullptr, *q = nullptr, *att = nullptr, *h1 = nullptr, *scores = nullptr;
    int ld_xn = 0, ld_att = 0, ld_h1 = 0;
    BatchTable *d_tab = nullptr, *h_tab = nullptr;
    VerifyGroupTable *d_groups = nullptr, *h_groups = nullptr;  // l2z_verify_batch: behind the table, in the same allocations
    VerifyTreeTable *d_tree = nullptr, *h_tree = nullptr;       // l2z_verify_tree: in the group table's place
    int *d_tokens_out = nullptr, *h_tokens_out = nullptr;
    hipEvent_t ev_in[kBatchMax] = {};
    hipEvent_t ev_done = nullptr;
    hipEvent_t ev_upload = nullptr;  // the last table copy: the pinned table may be rewritten once it has completed
    float *smp = nullptr;            // l2z_sample_batch: kBatchMax rows of sample_scratch_floats(vocab) (on first use)
    size_t smp_stride = 0;
    // l2z_verify (on the runstate's first call): the [kBatchMax, vocab] logits matrix, the attention partials
    // ([kBatchMax, n_heads, v_seg_cap, head_size] and [..., 2]), next[0 .. n) | accepted on the device and pinned
    float *v_logits = nullptr, *v_part_o = nullptr, *v_part_ml = nullptr;
    int *d_vout = nullptr, *h_vout = nullptr;  // 3 * kBatchMax ints (l2z_verify_batch: next[0 .. rows) | accepted[0 .. n);
                                               // l2z_verify_tree: next[0 .. n) | accepted | path[0 .. accepted])
    int v_seg_cap = 0, v_rows = 0;   // v_rows: rows of the last call (l2z_verify_logits_read)
};

void batch_free(l2z_runstate *s)
{
    BatchScratch *b = s->bt;
    if (b == nullptr) return;
    void *ptrs[] = {b->x, b->xn, b->q, b->att, b->h1, b->scores, b->d_tab, b->d_tokens_out, b->smp,
                    b->v_logits, b->v_part_o, b->v_part_ml, b->d_vout};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (b->h_tab) (void)hipHostFree(b->h_tab);
    if (b->h_tokens_out) (void)hipHostFree(b->h_tokens_out);
    if (b->h_vout) (void)hipHostFree(b->h_vout);
    for (hipEvent_t e : b->ev_in)
        if (e) (void)hipEventDestroy(e);
    if (b->ev_done) (void)hipEventDestroy(b->ev_done);
    if (b->ev_upload) (void)hipEventDestroy(b->ev_upload);
    delete b;
    s->bt = nullptr;
}

namespace {

// what follows the step's table in its allocations: the row groups of l2z_verify_batch or the tree of l2z_verify_tree
constexpr size_t kTabExtra = std::max(sizeof(VerifyGroupTable), sizeof(VerifyTreeTable));

// Row pitch of the activation matrices the GEMMs read: rounded up to 256 floats, at least 768, the pad columns zero and
// never written (the short-prompt forms multiply whole 256-k stages, at least three: prefill_common.h pad_k)
int bt_ld(int n)
{
    const int r = (n + 255) / 256 * 256;
    return r < 768 ? 768 : r;
}

int batch_alloc(l2z_runstate *s)
{
    if (s->bt != nullptr) return L2Z_OK;
    const l2z_config &c = s->cfg;
    BatchScratch *b = new BatchScratch();
    s->bt = b;  // freed with the runstate whatever happens below
    b->ld_xn = bt_ld(c.dim); b->ld_att = bt_ld(c.dim); b->ld_h1 = bt_ld(c.hidden_dim);
    const size_t R = kBatchMax;
    struct { void **p; size_t bytes; } want[] = {
        {(void **)&b->x, R * c.dim * 4}, {(void **)&b->xn, R * b->ld_xn * 4}, {(void **)&b->q, R * c.dim * 4},
        {(void **)&b->att, R * b->ld_att * 4}, {(void **)&b->h1, R * b->ld_h1 * 4},
        {(void **)&b->scores, R * (size_t)c.n_heads * c.seq_len * 4},
        {(void **)&b->d_tab, sizeof(BatchTable) + kTabExtra}, {(void **)&b->d_tokens_out, R * 4}};
    for (auto &w : want) {
        const hipError_t e = hipMalloc(w.p, w.bytes);
        if (e != hipSuccess) {
            *w.p = nullptr;
            set_error("batched step scratch allocation (%zu bytes) failed: %s", w.bytes, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? L2Z_ERR_OOM : L2Z_ERR_HIP;
        }
    }
    L2Z_HIP(hipHostMalloc((void **)&b->h_tab, sizeof(BatchTable) + kTabExtra, hipHostMallocDefault));
    b->d_groups = (VerifyGroupTable *)(b->d_tab + 1);
    b->h_groups = (VerifyGroupTable *)(b->h_tab + 1);
    b->d_tree = (VerifyTreeTable *)(b->d_tab + 1);
    b->h_tree = (VerifyTreeTable *)(b->h_tab + 1);
    L2Z_HIP(hipHostMalloc((void **)&b->h_tokens_out, R * 4, hipHostMallocDefault));
    for (hipEvent_t &e : b->ev_in) L2Z_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    L2Z_HIP(hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming));
    L2Z_HIP(hipEventCreateWithFlags(&b->ev_upload, hipEventDisableTiming));
    // the pad columns are multiplied against whatever follows a W row: zeros, once
    L2Z_HIP(hipMemset(b->xn, 0, R * b->ld_xn * 4));
    L2Z_HIP(hipMemset(b->att, 0, R * b->ld_att * 4));
    L2Z_HIP(hipMemset(b->h1, 0, R * b->ld_h1 * 4));
    return L2Z_OK;
}

int no_device_check()
{
    int nd = 0;
    const hipError_t e = hipGetDeviceCount(&nd);
    L2Z_CHECK(e == hipSuccess && nd > 0, L2Z_ERR_NO_DEVICE, "no HIP device available; this library has no CPU fallback");
    return L2Z_OK;
}

// the runstates of one call: non-null, pairwise distinct, unsharded, on one device, all made with *c (c: states[0]'s
// when the call names no config)
int check_states(const char *fn, int n, l2z_runstate *const *states, const l2z_config *c)
{
    L2Z_CHECK(n >= 1 && n <= kBatchMax, L2Z_ERR_INVALID, "%s: n = %d outside [1, %d]", fn, n, kBatchMax);
    L2Z_CHECK(states != nullptr, L2Z_ERR_INVALID, "%s: null runstate array", fn);
    for (int i = 0; i < n; i++) {
        const l2z_runstate *s = states[i];
        L2Z_CHECK(s != nullptr, L2Z_ERR_INVALID, "%s: states[%d] is null", fn, i);
        for (int j = 0; j < i; j++)
            L2Z_CHECK(states[j] != s, L2Z_ERR_INVALID, "%s: states[%d] and states[%d] are the same runstate", fn, j, i);
        L2Z_CHECK(s->comm == nullptr && s->sh.world == 1, L2Z_ERR_INVALID, "%s: states[%d] is a shard (shard groups are not batched)", fn, i);
        L2Z_CHECK(memcmp(c != nullptr ? c : &states[0]->cfg, &s->cfg, sizeof(l2z_config)) == 0, L2Z_ERR_INVALID,
                  "%s: states[%d] was made with another config", fn, i);
        L2Z_CHECK(s->device == states[0]->device, L2Z_ERR_INVALID, "%s: states[%d] is on device %d, states[0] on %d", fn, i,
                  s->device, states[0]->device);
    }
    return L2Z_OK;
}

// the pass waits for everything already queued on every runstate's stream
int join_streams(BatchScratch *b, int n, l2z_runstate *const *states)
{
    hipStream_t st = states[0]->stream;
    for (int i = 1; i < n; i++) {
        L2Z_HIP(hipEventRecord(b->ev_in[i], states[i]->stream));
        L2Z_HIP(hipStreamWaitEvent(st, b->ev_in[i], 0));
    }
    return L2Z_OK;
}

// ... and every runstate's stream waits for the pass
int release_streams(BatchScratch *b, int n, l2z_runstate *const *states)
{
    L2Z_HIP(hipEventRecord(b->ev_done, states[0]->stream));
    for (int i = 1; i < n; i++) L2Z_HIP(hipStreamWaitEvent(states[i]->stream, b->ev_done, 0));
    return L2Z_OK;
}

// the table of this call -> the device, one copy from the pinned buffer (rewritten only once the last copy is done)
int upload_table(BatchScratch *b, const BatchTable &t, hipStream_t st)
{
    L2Z_HIP(hipEventSynchronize(b->ev_upload));
    memcpy(b->h_tab, &t, sizeof t);
    L2Z_HIP(hipMemcpyAsync(b->d_tab, b->h_tab, sizeof t, hipMemcpyHostToDevice, st));
    L2Z_HIP(hipEventRecord(b->ev_upload, st));
    return L2Z_OK;
}

// ... and the row groups of an l2z_verify_batch call behind it, still one copy
int upload_tables(BatchScratch *b, const BatchTable &t, const VerifyGroupTable &g, hipStream_t st)
{
    static_assert(sizeof(BatchTable) % alignof(VerifyGroupTable) == 0, "the group table sits right behind the step's table");
    L2Z_HIP(hipEventSynchronize(b->ev_upload));
    memcpy(b->h_tab, &t, sizeof t);
    memcpy(b->h_groups, &g, sizeof g);
    L2Z_HIP(hipMemcpyAsync(b->d_tab, b->h_tab, sizeof t + sizeof g, hipMemcpyHostToDevice, st));
    L2Z_HIP(hipEventRecord(b->ev_upload, st));
    return L2Z_OK;
}

// ... or the tree of an l2z_verify_tree call
int upload_tables(BatchScratch *b, const BatchTable &t, const VerifyTreeTable &g, hipStream_t st)
{
    static_assert(sizeof(BatchTable) % alignof(VerifyTreeTable) == 0, "the tree table sits right behind the step's table");
    L2Z_HIP(hipEventSynchronize(b->ev_upload));
    memcpy(b->h_tab, &t, sizeof t);
    memcpy(b->h_tree, &g, sizeof g);
    L2Z_HIP(hipMemcpyAsync(b->d_tab, b->h_tab, sizeof t + sizeof g, hipMemcpyHostToDevice, st));
    L2Z_HIP(hipEventRecord(b->ev_upload, st));
    return L2Z_OK;
}

GemmArgs gemm(const float *x, int ldx, const float *w, int ldw, int N, int K, int P)
{
    GemmArgs a = {};
    a.x = x; a.ldx = ldx; a.w = w; a.ldw = ldw; a.N = N; a.K = K; a.P = P; a.n_scale = 1;
    return a;
}

// One step of n sequences on states[0]'s stream.  Every product is the one-tile short-prompt form at P = n whatever n
// is (launch_batch_skinny): a row's bits do not depend on n, on the other rows, or on its place in the batch.
// verify_pos0 >= 0 (l2z_verify): the rows are positions verify_pos0 .. of s0's own sequence, and attention is the
// multi-query position-split form over s0's cache (verify.hip) instead of one block per (head, row).
// vb_groups > 0 (l2z_verify_batch): the rows are the groups of b->d_groups, each on its own sequence's cache; attention is
// that form per group in one launch (verify_batch.hip), vb_segments = the deepest group's segment count.
// tree_depth >= 0 beside verify_pos0 >= 0 (l2z_verify_tree): the rows are the nodes of b->d_tree, the deepest tree_depth
// edges from the root, on s0's cache; attention is that form with every row on its own path (verify_tree.hip).
int batch_step(int n, const l2z_config &c, l2z_runstate *s0, const l2z_weights *w, BatchScratch *b, int verify_pos0 = -1,
               int vb_groups = 0, int vb_segments = 0, int tree_depth = -1)
{
    hipStream_t st = s0->stream;
    const int dim = c.dim, hid = c.hidden_dim, hs = dim / c.n_heads, kvd = hs * c.n_kv_heads;
    const BatchTable *tab = b->d_tab;
    L2Z_HIP(launch_prefill_embed(b->x, w->tok_emb, tab->tokens, dim, n, st));  // :295
    for (int l = 0; l < c.n_layers; l++) {
        const size_t layer_off = (size_t)l * c.seq_len * kvd;
        L2Z_HIP(launch_prefill_rmsnorm(b->xn, b->ld_xn, b->x, w->rms_att + (size_t)l * dim, dim, n, st));  // :305
        {   // q (:308-351): RoPE at each row's own position
            GemmArgs a = gemm(b->xn, b->ld_xn, w->wq + (size_t)l * dim * dim, dim, dim, dim, n);
            a.out = b->q; a.ldo = dim; a.rope = s0->rope; a.head_size = hs; a.row_pos = tab->pos;
            L2Z_HIP(launch_batch_skinny(G_ROPE_ROWS, a, st));
        }
        {   // k | v (:354-358) into each row's own caches, row = its position
            GemmArgs a = gemm(b->xn, b->ld_xn, w->wk + (size_t)l * kvd * dim, dim, kvd, dim, n);
            a.w2 = w->wv + (size_t)l * kvd * dim;
            a.rope = s0->rope; a.head_size = hs; a.ldkv = kvd; a.kv_head_stride = (size_t)c.seq_len * hs;
            a.row_pos = tab->pos; a.row_kc = tab->kc; a.row_vc = tab->vc; a.layer_off = layer_off;
            L2Z_HIP(launch_batch_skinny(G_QKV_ROWS, a, st));
        }
        if (vb_groups > 0) {  // :361-389, flash form per group
            VerifyBatchAttnArgs a = {};
            a.q = b->q; a.ldq = dim; a.out = b->att; a.ldo = b->ld_att; a.part_o = b->v_part_o; a.part_ml = b->v_part_ml;
            a.tab = tab; a.groups = b->d_groups; a.layer_off = layer_off; a.kv_head_stride = (size_t)c.seq_len * hs;
            a.n_heads = c.n_heads; a.kv_mul = c.n_heads / c.n_kv_heads; a.head_size = hs; a.seg_cap = b->v_seg_cap;
            L2Z_HIP(launch_verify_batch_attention(a, vb_groups, vb_segments, st));
            L2Z_HIP(launch_verify_batch_combine(a, n, st));
        } else if (verify_pos0 >= 0 && tree_depth >= 0) {  // :361-389, flash form along each row's path
            VerifyTreeAttnArgs a = {};
            a.q = b->q; a.ldq = dim; a.out = b->att; a.ldo = b->ld_att; a.part_o = b->v_part_o; a.part_ml = b->v_part_ml;
            a.kc = s0->key_cache + layer_off; a.vc = s0->value_cache + layer_off; a.tree = b->d_tree;
            a.kv_head_stride = (size_t)c.seq_len * hs;
            a.n_heads = c.n_heads; a.kv_mul = c.n_heads / c.n_kv_heads; a.head_size = hs; a.seg_cap = b->v_seg_cap;
            a.pos0 = verify_pos0;
            L2Z_HIP(launch_verify_tree_attention(a, n, tree_depth, st));
            L2Z_HIP(launch_verify_tree_combine(a, n, tree_depth, st));
        } else if (verify_pos0 >= 0) {  // :361-389, flash form
            VerifyAttnArgs a = {};
            a.q = b->q; a.ldq = dim; a.out = b->att; a.ldo = b->ld_att; a.part_o = b->v_part_o; a.part_ml = b->v_part_ml;
            a.kc = s0->key_cache + layer_off; a.vc = s0->value_cache + layer_off;
            a.kv_head_stride = (size_t)c.seq_len * hs;
            a.n_heads = c.n_heads; a.kv_mul = c.n_heads / c.n_kv_heads; a.head_size = hs; a.seg_cap = b->v_seg_cap;
            a.pos0 = verify_pos0;
            L2Z_HIP(launch_verify_attention(a, n, st));
            L2Z_HIP(launch_verify_combine(a, n, st));
        } else {  // :361-389
            BatchAttnArgs a = {};
            a.q = b->q; a.ldq = dim; a.out = b->att; a.ldo = b->ld_att; a.scores = b->scores; a.tab = tab;
            a.layer_off = layer_off; a.kv_head_stride = (size_t)c.seq_len * hs;
            a.n_heads = c.n_heads; a.kv_mul = c.n_heads / c.n_kv_heads; a.head_size = hs; a.seq_len = c.seq_len;
            L2Z_HIP(launch_batch_attention(a, n, st));
        }
        {   // :392-395
            GemmArgs a = gemm(b->att, b->ld_att, w->wo + (size_t)l * dim * dim, dim, dim, dim, n);
            a.out = b->x; a.ldo = dim; a.res = b->x; a.ldres = dim;
            L2Z_HIP(launch_batch_skinny(G_RESID, a, st));
        }
        L2Z_HIP(launch_prefill_rmsnorm(b->xn, b->ld_xn, b->x, w->rms_ffn + (size_t)l * dim, dim, n, st));  // :398
        {   // :405-416: W1 | W3 (rows 2 dim apart in their shared slot) with silu(a) * b in the epilogue
            GemmArgs a = gemm(b->xn, b->ld_xn, w->w1 + (size_t)l * hid * 2 * dim, 2 * dim, hid, dim, n);
            a.w2 = w->w3 + (size_t)l * hid * 2 * dim;
            a.out = b->h1; a.ldo = b->ld_h1;
            L2Z_HIP(launch_batch_skinny(G_SWIGLU, a, st));
        }
        {   // :419-422
            GemmArgs a = gemm(b->h1, b->ld_h1, w->w2 + (size_t)l * dim * hid, hid, dim, hid, n);
            a.out = b->x; a.ldo = dim; a.res = b->x; a.ldres = dim;
            L2Z_HIP(launch_batch_skinny(G_RESID, a, st));
        }
    }
    L2Z_HIP(launch_prefill_rmsnorm(b->xn, b->ld_xn, b->x, w->rms_final, dim, n, st));  // :426
    {   // :429: each row's logits straight into its runstate
        GemmArgs a = gemm(b->xn, b->ld_xn, w->wcls, dim, c.vocab_size, dim, n);
        a.row_out = tab->logits;
        L2Z_HIP(launch_batch_skinny(G_OUT_ROWS, a, st));
    }
    return L2Z_OK;
}

}  // namespace

// the same rules for the batched prompt pass (prefill_batch_host.cpp)
int batch_no_device_check() { return no_device_check(); }
int batch_check_states(const char *fn, int n, l2z_runstate *const *states, const l2z_config *c) { return check_states(fn, n, states, c); }
int batch_join_streams(int n, l2z_runstate *const *states)
{
    L2Z_TRY(batch_alloc(states[0]));
    return join_streams(states[0]->bt, n, states);
}
int batch_release_streams(int n, l2z_runstate *const *states) { return release_streams(states[0]->bt, n, states); }

}  // namespace l2z

using namespace l2z;

extern "C" int l2z_transformer_batch(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                                     l2z_runstate *const *states, const l2z_weights *w)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && pos != nullptr && config != nullptr && w != nullptr, L2Z_ERR_INVALID,
              "l2z_transformer_batch: null argument");
    L2Z_TRY(check_states("l2z_transformer_batch", n, states, config));
    for (int i = 0; i < n; i++) {
        L2Z_TRY(check_pair(config, states[i], w));
        L2Z_CHECK(pos[i] >= 0 && pos[i] < config->seq_len, L2Z_ERR_STATE, "l2z_transformer_batch: pos[%d] = %d outside [0,%d)", i,
                  pos[i], config->seq_len);
        L2Z_CHECK(tokens[i] >= 0 && tokens[i] < config->vocab_size, L2Z_ERR_STATE,
                  "l2z_transformer_batch: tokens[%d] = %d out of vocabulary", i, tokens[i]);
    }
    L2Z_TRY(prefill_check(config, states[0]));
    L2Z_CHECK(states[0]->sh.hs <= 256, L2Z_ERR_INVALID, "l2z_transformer_batch: head_size above 256");
    L2Z_HIP(hipSetDevice(states[0]->device));
    L2Z_TRY(batch_alloc(states[0]));
    BatchScratch *b = states[0]->bt;
    BatchTable t = {};
    for (int i = 0; i < n; i++) {
        t.tokens[i] = tokens[i];
        t.pos[i] = pos[i];
        t.kc[i] = states[i]->key_cache;
        t.vc[i] = states[i]->value_cache;
        t.logits[i] = states[i]->logits;
    }
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(upload_table(b, t, states[0]->stream));
    L2Z_TRY(batch_step(n, *config, states[0], w, b));
    L2Z_TRY(release_streams(b, n, states));
    for (int i = 0; i < n; i++) {
        l2z_runstate *s = states[i];
        s->n_part = 0;  // l2z_argmax scans the logits: the classifier left no per-block candidates
        s->logits_partial = false;
        s->host_pos = pos[i] + 1;
    }
    return L2Z_OK;
}

extern "C" int l2z_argmax_batch(int n, l2z_runstate *const *states, int32_t *out_tokens)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out_tokens != nullptr, L2Z_ERR_INVALID, "l2z_argmax_batch: null argument");
    L2Z_TRY(check_states("l2z_argmax_batch", n, states, nullptr));
    L2Z_HIP(hipSetDevice(states[0]->device));
    L2Z_TRY(batch_alloc(states[0]));
    BatchScratch *b = states[0]->bt;
    BatchTable t = {};
    for (int i = 0; i < n; i++) t.logits[i] = states[i]->logits;
    hipStream_t st = states[0]->stream;
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(upload_table(b, t, st));
    L2Z_HIP(launch_batch_argmax(b->d_tab, states[0]->cfg.vocab_size, b->d_tokens_out, n, st));
    L2Z_HIP(hipMemcpyAsync(b->h_tokens_out, b->d_tokens_out, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_tokens, b->h_tokens_out, (size_t)n * 4);
    return L2Z_OK;
}

namespace l2z {
namespace {

int sample_alloc(l2z_runstate *s)
{
    BatchScratch *b = s->bt;
    if (b->smp != nullptr) return L2Z_OK;
    const size_t stride = sample_scratch_floats(s->cfg.vocab_size), bytes = kBatchMax * stride * 4;
    const hipError_t e = hipMalloc(&b->smp, bytes);
    if (e != hipSuccess) {
        b->smp = nullptr;
        set_error("l2z_sample_batch scratch allocation (%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? L2Z_ERR_OOM : L2Z_ERR_HIP;
    }
    b->smp_stride = stride;
    return L2Z_OK;
}

// l2z_sample_batch's checks, table and launch on states[0]'s stream (no copy back)
int sample_enqueue(int n, l2z_runstate *const *states, const float *temperature, const float *top_p, const float *coins)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(temperature != nullptr && top_p != nullptr && coins != nullptr, L2Z_ERR_INVALID,
              "l2z_sample_batch: null argument");
    L2Z_TRY(check_states("l2z_sample_batch", n, states, nullptr));
    for (int i = 0; i < n; i++) {
        L2Z_CHECK(std::isfinite(temperature[i]) && temperature[i] >= 0.0f, L2Z_ERR_INVALID,
                  "l2z_sample_batch: temperature[%d] = %g (finite, >= 0)", i, (double)temperature[i]);
        L2Z_CHECK(top_p[i] >= 0.0f && top_p[i] <= 1.0f, L2Z_ERR_INVALID, "l2z_sample_batch: top_p[%d] = %g outside [0, 1]", i,
                  (double)top_p[i]);
        L2Z_CHECK(coins[i] >= 0.0f && coins[i] < 1.0f, L2Z_ERR_INVALID, "l2z_sample_batch: coins[%d] = %g outside [0, 1)", i,
                  (double)coins[i]);
    }
    L2Z_HIP(hipSetDevice(states[0]->device));
    L2Z_TRY(batch_alloc(states[0]));
    L2Z_TRY(sample_alloc(states[0]));
    BatchScratch *b = states[0]->bt;
    BatchTable t = {};
    for (int i = 0; i < n; i++) {
        t.logits[i] = states[i]->logits;
        t.temperature[i] = temperature[i];
        t.top_p[i] = top_p[i];
        t.coin[i] = coins[i];
    }
    hipStream_t st = states[0]->stream;
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(upload_table(b, t, st));
    SampleArgs a = {};
    a.tab = b->d_tab; a.scratch = b->smp; a.row_stride = b->smp_stride; a.vocab = states[0]->cfg.vocab_size;
    a.out = b->d_tokens_out;
    L2Z_HIP(launch_sample_batch(a, n, st));
    return L2Z_OK;
}

}  // namespace
}  // namespace l2z

extern "C" int l2z_sample_batch(int n, l2z_runstate *const *states, const float *temperature, const float *top_p,
                                const float *coins, int32_t *out_tokens)
{
    L2Z_CHECK(out_tokens != nullptr, L2Z_ERR_INVALID, "l2z_sample_batch: null argument");
    L2Z_TRY(sample_enqueue(n, states, temperature, top_p, coins));
    BatchScratch *b = states[0]->bt;
    hipStream_t st = states[0]->stream;
    L2Z_HIP(hipMemcpyAsync(b->h_tokens_out, b->d_tokens_out, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(release_streams(b, n, states));
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_tokens, b->h_tokens_out, (size_t)n * 4);
    return L2Z_OK;
}

extern "C" int l2z_runstate_fork(l2z_runstate *dst, const l2z_runstate *src, int n_pos)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(dst != nullptr && src != nullptr, L2Z_ERR_INVALID, "l2z_runstate_fork: null runstate");
    L2Z_CHECK(dst != src, L2Z_ERR_INVALID, "l2z_runstate_fork: dst and src are the same runstate");
    L2Z_CHECK(dst->comm == nullptr && dst->sh.world == 1 && src->comm == nullptr && src->sh.world == 1, L2Z_ERR_INVALID,
              "l2z_runstate_fork: shard runstates are not forked");
    L2Z_CHECK(memcmp(&dst->cfg, &src->cfg, sizeof(l2z_config)) == 0, L2Z_ERR_INVALID,
              "l2z_runstate_fork: dst was made with another config");
    L2Z_CHECK(dst->device == src->device, L2Z_ERR_INVALID, "l2z_runstate_fork: dst is on device %d, src on %d", dst->device,
              src->device);
    const l2z_config &c = src->cfg;
    L2Z_CHECK(n_pos >= 0 && n_pos <= c.seq_len, L2Z_ERR_STATE, "l2z_runstate_fork: n_pos = %d outside [0, %d]", n_pos,
              c.seq_len);
    L2Z_HIP(hipSetDevice(src->device));
    hipEvent_t ev_src = nullptr, ev_dst = nullptr;
    L2Z_HIP(hipEventCreateWithFlags(&ev_src, hipEventDisableTiming));
    int rc = L2Z_OK;
    auto hip = [&rc](hipError_t e, const char *what) {
        if (rc == L2Z_OK && e != hipSuccess) {
            set_error("l2z_runstate_fork: %s: %s", what, hipGetErrorString(e));
            rc = L2Z_ERR_HIP;
        }
    };
    hip(hipEventCreateWithFlags(&ev_dst, hipEventDisableTiming), "hipEventCreate");
    // dst's stream waits for what src's has queued (the rows and logits being copied) ...
    hip(hipEventRecord(ev_src, src->stream), "hipEventRecord");
    hip(hipStreamWaitEvent(dst->stream, ev_src, 0), "hipStreamWaitEvent");
    // ... the caches are head-major [layer][kv head][seq_len][head_size]: positions 0 .. n_pos - 1 are one
    // run of n_pos * head_size floats per (layer, kv head), seq_len * head_size floats apart
    const size_t hs = (size_t)c.dim / c.n_heads, pitch = (size_t)c.seq_len * hs * 4, width = (size_t)n_pos * hs * 4;
    const size_t rows = (size_t)c.n_layers * c.n_kv_heads;
    if (n_pos > 0 && rc == L2Z_OK) {
        hip(hipMemcpy2DAsync(dst->key_cache, pitch, src->key_cache, pitch, width, rows, hipMemcpyDeviceToDevice, dst->stream),
            "key cache copy");
        hip(hipMemcpy2DAsync(dst->value_cache, pitch, src->value_cache, pitch, width, rows, hipMemcpyDeviceToDevice,
                             dst->stream),
            "value cache copy");
    }
    if (rc == L2Z_OK)
        hip(hipMemcpyAsync(dst->logits, src->logits, (size_t)c.vocab_size * 4, hipMemcpyDeviceToDevice, dst->stream),
            "logits copy");
    // ... and src's stream waits for the copies: its next step overwrites the logits they read
    hip(hipEventRecord(ev_dst, dst->stream), "hipEventRecord");
    hip(hipStreamWaitEvent(src->stream, ev_dst, 0), "hipStreamWaitEvent");
    (void)hipEventDestroy(ev_src);  // released by the runtime once the streams are past them
    if (ev_dst) (void)hipEventDestroy(ev_dst);
    if (rc != L2Z_OK) return rc;
    dst->n_part = 0;  // l2z_argmax scans the copied logits, not dst's own classifier candidates
    dst->logits_partial = false;
    dst->host_pos = n_pos;
    return L2Z_OK;
}

// Testing support (include/llama2_hip_test.h): place exact logits in a runstate (vocab_size floats), queued on its stream
extern "C" int l2z_logits_write(l2z_runstate *s, const float *logits)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(s != nullptr && logits != nullptr, L2Z_ERR_INVALID, "l2z_logits_write: null argument");
    L2Z_CHECK(s->comm == nullptr && s->sh.world == 1, L2Z_ERR_INVALID, "l2z_logits_write: shard runstate");
    L2Z_HIP(hipSetDevice(s->device));
    L2Z_HIP(hipMemcpyAsync(s->logits, logits, (size_t)s->cfg.vocab_size * 4, hipMemcpyHostToDevice, s->stream));
    L2Z_HIP(hipStreamSynchronize(s->stream));
    s->n_part = 0;
    s->logits_partial = false;
    return L2Z_OK;
}

// Testing support: `iters` l2z_sample_batch launches back to back (no copy back), timed by device events on the
// launches' stream (scripts/sample_bench.py)
extern "C" int l2z_sample_time(int n, l2z_runstate *const *states, const float *temperature, const float *top_p,
                               const float *coins, int iters, double *out_ms)
{
    L2Z_CHECK(iters >= 1 && out_ms != nullptr, L2Z_ERR_INVALID, "l2z_sample_time: bad arguments");
    L2Z_TRY(sample_enqueue(n, states, temperature, top_p, coins));  // validates, allocates, warms up
    hipStream_t st = states[0]->stream;
    hipEvent_t e0, e1;
    L2Z_HIP(hipEventCreate(&e0));
    L2Z_HIP(hipEventCreate(&e1));
    int rc = L2Z_OK;
    if (hipEventRecord(e0, st) != hipSuccess) rc = L2Z_ERR_HIP;
    BatchScratch *b = states[0]->bt;
    SampleArgs a = {};
    a.tab = b->d_tab; a.scratch = b->smp; a.row_stride = b->smp_stride; a.vocab = states[0]->cfg.vocab_size;
    a.out = b->d_tokens_out;
    for (int i = 0; i < iters && rc == L2Z_OK; i++)
        if (launch_sample_batch(a, n, st) != hipSuccess) rc = L2Z_ERR_HIP;
    float ms = 0.0f;
    if (rc == L2Z_OK && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                         hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
        rc = L2Z_ERR_HIP;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc == L2Z_OK) *out_ms = ms / iters;
    return rc;
}

// Testing support (include/llama2_hip_test.h): `iters` batched steps back to back, timed by device events on the pass's
// stream (scripts/batch_bench.py)
extern "C" int l2z_batch_time(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                              l2z_runstate *const *states, const l2z_weights *w, int iters, double *out_ms)
{
    L2Z_CHECK(iters >= 1 && out_ms != nullptr, L2Z_ERR_INVALID, "l2z_batch_time: bad arguments");
    L2Z_TRY(l2z_transformer_batch(n, tokens, pos, config, states, w));  // validates, allocates
    hipStream_t st = states[0]->stream;
    hipEvent_t e0, e1;
    L2Z_HIP(hipEventCreate(&e0));
    L2Z_HIP(hipEventCreate(&e1));
    int rc = L2Z_OK;
    if (hipEventRecord(e0, st) != hipSuccess) rc = L2Z_ERR_HIP;
    for (int i = 0; i < iters && rc == L2Z_OK; i++) rc = l2z_transformer_batch(n, tokens, pos, config, states, w);
    float ms = 0.0f;
    if (rc == L2Z_OK && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                         hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
        rc = L2Z_ERR_HIP;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc == L2Z_OK) *out_ms = ms / iters;
    return rc;
}

// ---- l2z_verify: n consecutive positions of ONE sequence in one sweep, and which guesses the model agrees with ----
namespace l2z {
namespace {

int verify_alloc(l2z_runstate *s)
{
    BatchScratch *b = s->bt;
    if (b->v_logits != nullptr && b->v_part_o != nullptr && b->v_part_ml != nullptr && b->d_vout != nullptr &&
        b->h_vout != nullptr)
        return L2Z_OK;
    const l2z_config &c = s->cfg;
    const size_t R = kBatchMax, segs = (size_t)verify_segments(c.seq_len), hs = (size_t)c.dim / c.n_heads;
    struct { void **p; size_t bytes; } want[] = {
        {(void **)&b->v_logits, R * (size_t)c.vocab_size * 4},
        {(void **)&b->v_part_o, R * c.n_heads * segs * hs * 4},
        {(void **)&b->v_part_ml, R * c.n_heads * segs * 2 * 4},
        {(void **)&b->d_vout, 3 * R * 4}};
    for (auto &w : want) {
        if (*w.p != nullptr) continue;
        const hipError_t e = hipMalloc(w.p, w.bytes);
        if (e != hipSuccess) {
            *w.p = nullptr;
            set_error("l2z_verify scratch allocation (%zu bytes) failed: %s", w.bytes, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? L2Z_ERR_OOM : L2Z_ERR_HIP;
        }
    }
    if (b->h_vout == nullptr) L2Z_HIP(hipHostMalloc((void **)&b->h_vout, 3 * R * 4, hipHostMallocDefault));
    b->v_seg_cap = (int)segs;
    return L2Z_OK;
}

// How a sampled pass draws its rows (l2z_verify_sample): row i is l2z_sample_batch's draw from z_i with coins[i]
struct VerifyDraw {
    float temperature, top_p;
    const float *coins;
};

// l2z_verify's checks (a refusal enqueues nothing), then the table, the pass, the verdict and its copy back on s's
// stream; no sync.  draw == nullptr: the greedy verdict; else the rows' ids are sample_batch_kernel's (temperature > 0).
int verify_enqueue(const char *fn, const int32_t *tokens, int n, int pos0, const l2z_config *config, l2z_runstate *s,
                   const l2z_weights *w, const VerifyDraw *draw = nullptr)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && config != nullptr && s != nullptr && w != nullptr, L2Z_ERR_INVALID, "%s: null argument",
              fn);
    L2Z_CHECK(n >= 1 && n <= kBatchMax, L2Z_ERR_INVALID, "%s: n_tokens = %d outside [1, %d]", fn, n, kBatchMax);
    L2Z_CHECK(s->comm == nullptr && s->sh.world == 1, L2Z_ERR_INVALID, "%s: the runstate is a shard", fn);
    L2Z_TRY(check_pair(config, s, w));
    L2Z_TRY(prefill_check(config, s));
    L2Z_CHECK(s->sh.hs <= 256, L2Z_ERR_INVALID, "%s: head_size above 256", fn);
    L2Z_CHECK(pos0 >= 0 && pos0 <= config->seq_len - n, L2Z_ERR_STATE, "%s: positions %d .. %d outside [0, %d)", fn, pos0,
              pos0 + n - 1, config->seq_len);
    for (int i = 0; i < n; i++)
        L2Z_CHECK(tokens[i] >= 0 && tokens[i] < config->vocab_size, L2Z_ERR_STATE, "%s: tokens[%d] = %d out of vocabulary", fn,
                  i, tokens[i]);
    if (draw != nullptr)  // l2z_sample_batch's rules
        for (int i = 0; i < n; i++)
            L2Z_CHECK(draw->coins[i] >= 0.0f && draw->coins[i] < 1.0f, L2Z_ERR_INVALID, "%s: coins[%d] = %g outside [0, 1)", fn,
                      i, (double)draw->coins[i]);
    L2Z_HIP(hipSetDevice(s->device));
    L2Z_TRY(batch_alloc(s));
    L2Z_TRY(verify_alloc(s));
    if (draw != nullptr) L2Z_TRY(sample_alloc(s));
    BatchScratch *b = s->bt;
    BatchTable t = {};
    for (int i = 0; i < n; i++) {
        t.tokens[i] = tokens[i];
        t.pos[i] = pos0 + i;
        t.kc[i] = s->key_cache;
        t.vc[i] = s->value_cache;
        t.logits[i] = b->v_logits + (size_t)i * config->vocab_size;
        if (draw != nullptr) {
            t.temperature[i] = draw->temperature;
            t.top_p[i] = draw->top_p;
            t.coin[i] = draw->coins[i];
        }
    }
    hipStream_t st = s->stream;
    L2Z_TRY(upload_table(b, t, st));
    L2Z_TRY(batch_step(n, *config, s, w, b, pos0));
    if (draw != nullptr) {  // the rows' draws by l2z_sample_batch's kernel, then the accept scan over them
        SampleArgs a = {};
        a.tab = b->d_tab; a.scratch = b->smp; a.row_stride = b->smp_stride; a.vocab = config->vocab_size;
        a.out = b->d_vout;
        L2Z_HIP(launch_sample_batch(a, n, st));
        L2Z_HIP(launch_verify_accept_ids(b->d_tab, b->v_logits, config->vocab_size, b->d_vout, s->logits, n, st));
    } else {
        L2Z_HIP(launch_verify_accept(b->d_tab, b->v_logits, config->vocab_size, b->d_vout, s->logits, n, st));
    }
    L2Z_HIP(hipMemcpyAsync(b->h_vout, b->d_vout, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, st));
    b->v_rows = n;
    s->n_part = 0;  // l2z_argmax scans the logits the verdict copied
    s->logits_partial = false;
    return L2Z_OK;
}

// l2z_verify_sample's own argument rules (before verify_enqueue's, which queue nothing either); *draw: what to pass on,
// nullptr at temperature 0 (the greedy verdict, l2z_verify's launches)
int verify_sample_args(float temperature, float top_p, const float *coins, VerifyDraw *store, const VerifyDraw **draw)
{
    L2Z_CHECK(std::isfinite(temperature) && temperature >= 0.0f, L2Z_ERR_INVALID,
              "l2z_verify_sample: temperature = %g (finite, >= 0)", (double)temperature);
    L2Z_CHECK(top_p >= 0.0f && top_p <= 1.0f, L2Z_ERR_INVALID, "l2z_verify_sample: top_p = %g outside [0, 1]", (double)top_p);
    L2Z_CHECK(temperature == 0.0f || coins != nullptr, L2Z_ERR_INVALID,
              "l2z_verify_sample: coins is NULL at temperature %g", (double)temperature);
    *store = VerifyDraw{temperature, top_p, coins};
    *draw = temperature == 0.0f ? nullptr : store;
    return L2Z_OK;
}

}  // namespace
}  // namespace l2z

extern "C" int l2z_verify(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
                          const l2z_weights *w, int32_t *out_next, int *out_accepted)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out_next != nullptr && out_accepted != nullptr, L2Z_ERR_INVALID, "l2z_verify: null argument");
    L2Z_TRY(verify_enqueue("l2z_verify", tokens, n_tokens, pos0, config, s, w));
    BatchScratch *b = s->bt;
    L2Z_HIP(hipStreamSynchronize(s->stream));
    memcpy(out_next, b->h_vout, (size_t)n_tokens * 4);
    *out_accepted = b->h_vout[n_tokens];
    s->host_pos = pos0 + *out_accepted + 1;
    return L2Z_OK;
}

extern "C" int l2z_verify_sample(const int32_t *tokens, int n_tokens, int pos0, float temperature, float top_p,
                                 const float *coins, const l2z_config *config, l2z_runstate *s, const l2z_weights *w,
                                 int32_t *out_next, int *out_accepted)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out_next != nullptr && out_accepted != nullptr, L2Z_ERR_INVALID, "l2z_verify_sample: null argument");
    VerifyDraw store;
    const VerifyDraw *draw = nullptr;
    L2Z_TRY(verify_sample_args(temperature, top_p, coins, &store, &draw));
    L2Z_TRY(verify_enqueue("l2z_verify_sample", tokens, n_tokens, pos0, config, s, w, draw));
    BatchScratch *b = s->bt;
    L2Z_HIP(hipStreamSynchronize(s->stream));
    memcpy(out_next, b->h_vout, (size_t)n_tokens * 4);
    *out_accepted = b->h_vout[n_tokens];
    s->host_pos = pos0 + *out_accepted + 1;
    return L2Z_OK;
}

// ---- l2z_verify_batch: the verify pass for the rows of several sequences in one sweep (include/llama2_hip_test.h) ----
extern "C" int l2z_verify_batch(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                                const float *temperature, const float *top_p, const float *coins, const l2z_config *config,
                                l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next, int32_t *out_accepted)
{
    const char *fn = "l2z_verify_batch";
    // ---- checks: a refusal enqueues nothing and changes no state ----
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && n_tokens != nullptr && pos0 != nullptr && config != nullptr && w != nullptr &&
                  out_next != nullptr && out_accepted != nullptr,
              L2Z_ERR_INVALID, "%s: null argument", fn);
    L2Z_TRY(check_states(fn, n, states, config));
    int R = 0;
    for (int j = 0; j < n; j++) {
        L2Z_CHECK(n_tokens[j] >= 1 && n_tokens[j] <= kBatchMax, L2Z_ERR_INVALID, "%s: n_tokens[%d] = %d outside [1, %d]", fn, j,
                  n_tokens[j], kBatchMax);
        R += n_tokens[j];
    }
    L2Z_CHECK(R <= kBatchMax, L2Z_ERR_INVALID, "%s: %d rows in all, above %d", fn, R, kBatchMax);
    for (int j = 0; j < n; j++) L2Z_TRY(check_pair(config, states[j], w));
    L2Z_TRY(prefill_check(config, states[0]));
    L2Z_CHECK(states[0]->sh.hs <= 256, L2Z_ERR_INVALID, "%s: head_size above 256", fn);
    bool sampled = false;  // any sequence at temperature > 0: the rows' ids are sample_batch_kernel's
    if (temperature != nullptr) {  // l2z_verify_sample's rules, per sequence
        L2Z_CHECK(top_p != nullptr, L2Z_ERR_INVALID, "%s: top_p is NULL beside a temperature array", fn);
        for (int j = 0, r = 0; j < n; r += n_tokens[j], j++) {
            L2Z_CHECK(std::isfinite(temperature[j]) && temperature[j] >= 0.0f, L2Z_ERR_INVALID,
                      "%s: temperature[%d] = %g (finite, >= 0)", fn, j, (double)temperature[j]);
            L2Z_CHECK(top_p[j] >= 0.0f && top_p[j] <= 1.0f, L2Z_ERR_INVALID, "%s: top_p[%d] = %g outside [0, 1]", fn, j,
                      (double)top_p[j]);
            if (temperature[j] == 0.0f) continue;
            sampled = true;
            L2Z_CHECK(coins != nullptr, L2Z_ERR_INVALID, "%s: coins is NULL at temperature[%d] = %g", fn, j, (double)temperature[j]);
            for (int i = 0; i < n_tokens[j]; i++)
                L2Z_CHECK(coins[r + i] >= 0.0f && coins[r + i] < 1.0f, L2Z_ERR_INVALID, "%s: coins[%d] = %g outside [0, 1)", fn,
                          r + i, (double)coins[r + i]);
        }
    }
    for (int j = 0, r = 0; j < n; r += n_tokens[j], j++) {
        L2Z_CHECK(pos0[j] >= 0 && pos0[j] <= config->seq_len - n_tokens[j], L2Z_ERR_STATE,
                  "%s: sequence %d: positions %d .. %lld outside [0, %d)", fn, j, pos0[j], (long long)pos0[j] + n_tokens[j] - 1,
                  config->seq_len);
        for (int i = 0; i < n_tokens[j]; i++)
            L2Z_CHECK(tokens[r + i] >= 0 && tokens[r + i] < config->vocab_size, L2Z_ERR_STATE,
                      "%s: sequence %d: tokens[%d] = %d out of vocabulary", fn, j, i, tokens[r + i]);
    }
    l2z_runstate *s0 = states[0];
    L2Z_HIP(hipSetDevice(s0->device));
    L2Z_TRY(batch_alloc(s0));
    L2Z_TRY(verify_alloc(s0));
    if (sampled) L2Z_TRY(sample_alloc(s0));
    BatchScratch *b = s0->bt;
    // ---- the step's table (a row per position) and the row groups (one per sequence) ----
    BatchTable t = {};
    VerifyGroupTable g = {};
    int segments = 1;
    for (int j = 0, r = 0; j < n; r += n_tokens[j], j++) {
        g.first[j] = r; g.count[j] = n_tokens[j]; g.pos0[j] = pos0[j];
        g.kc[j] = states[j]->key_cache; g.vc[j] = states[j]->value_cache; g.dst[j] = states[j]->logits;
        segments = std::max(segments, (pos0[j] + n_tokens[j] - 1) / kVerifySeg + 1);
        for (int i = 0; i < n_tokens[j]; i++) {
            t.tokens[r + i] = tokens[r + i];
            t.pos[r + i] = pos0[j] + i;
            t.kc[r + i] = states[j]->key_cache;
            t.vc[r + i] = states[j]->value_cache;
            t.logits[r + i] = b->v_logits + (size_t)(r + i) * config->vocab_size;
            if (sampled) {  // a temperature-0 sequence's rows are arg-maxed by the sampler's kernel: no coin is read
                t.temperature[r + i] = temperature[j];
                t.top_p[r + i] = top_p[j];
                t.coin[r + i] = temperature[j] > 0.0f ? coins[r + i] : 0.0f;
            }
        }
    }
    hipStream_t st = s0->stream;
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(upload_tables(b, t, g, st));
    L2Z_TRY(batch_step(R, *config, s0, w, b, -1, n, segments));
    if (sampled) {
        SampleArgs a = {};
        a.tab = b->d_tab; a.scratch = b->smp; a.row_stride = b->smp_stride; a.vocab = config->vocab_size;
        a.out = b->d_vout;
        L2Z_HIP(launch_sample_batch(a, R, st));
    } else {
        L2Z_HIP(launch_verify_batch_argmax(b->v_logits, config->vocab_size, b->d_vout, R, st));
    }
    L2Z_HIP(launch_verify_batch_accept(b->d_tab, b->d_groups, b->v_logits, config->vocab_size, b->d_vout, R, n, st));
    L2Z_HIP(hipMemcpyAsync(b->h_vout, b->d_vout, (size_t)(R + n) * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(release_streams(b, n, states));
    for (int j = 0; j < n; j++) {
        l2z_runstate *s = states[j];
        s->n_part = 0;  // l2z_argmax scans the logits the verdict copied
        s->logits_partial = false;
        if (s->bt != nullptr) s->bt->v_rows = j == 0 ? R : 0;  // l2z_verify_logits_read: the matrix is states[0]'s
    }
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_next, b->h_vout, (size_t)R * 4);
    for (int j = 0; j < n; j++) {
        out_accepted[j] = b->h_vout[R + j];
        states[j]->host_pos = pos0[j] + out_accepted[j] + 1;
    }
    return L2Z_OK;
}

// ---- l2z_verify_tree: the verify pass for a TREE of guesses on one sequence (include/llama2_hip_test.h) ----
namespace l2z {
namespace {

// l2z_verify_tree's checks (a refusal enqueues nothing), then the tables, the pass, the verdict, the compaction and the
// verdict's copy back on s's stream; no sync.
int verify_tree_enqueue(const int32_t *tokens, const int32_t *parent, int n, int pos0, float temperature, float top_p,
                        const float *coins, const l2z_config *config, l2z_runstate *s, const l2z_weights *w)
{
    const char *fn = "l2z_verify_tree";
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && parent != nullptr && config != nullptr && s != nullptr && w != nullptr, L2Z_ERR_INVALID,
              "%s: null argument", fn);
    L2Z_CHECK(n >= 1 && n <= kBatchMax, L2Z_ERR_INVALID, "%s: n_nodes = %d outside [1, %d]", fn, n, kBatchMax);
    L2Z_CHECK(parent[0] == -1, L2Z_ERR_INVALID, "%s: parent[0] = %d (the root's is -1)", fn, parent[0]);
    VerifyTreeTable g = {};
    int max_depth = 0;
    g.parent[0] = -1;
    g.below[0] = 1u;
    g.level[0] = 1u;
    for (int i = 1; i < n; i++) {
        L2Z_CHECK(parent[i] >= 0 && parent[i] < i, L2Z_ERR_INVALID, "%s: parent[%d] = %d outside [0, %d)", fn, i, parent[i], i);
        g.parent[i] = parent[i];
        g.depth[i] = g.depth[parent[i]] + 1;
        g.level[g.depth[i]] |= 1u << i;
        for (int j = i; j >= 0; j = g.parent[j]) g.below[j] |= 1u << i;
        max_depth = std::max(max_depth, g.depth[i]);
    }
    for (int i = 1; i < n; i++)
        for (int j = 1; j < i; j++)
            L2Z_CHECK(parent[i] != parent[j] || tokens[i] != tokens[j], L2Z_ERR_INVALID,
                      "%s: nodes %d and %d are siblings with one token (%d)", fn, j, i, tokens[i]);
    L2Z_CHECK(s->comm == nullptr && s->sh.world == 1, L2Z_ERR_INVALID, "%s: the runstate is a shard", fn);
    L2Z_TRY(check_pair(config, s, w));
    L2Z_TRY(prefill_check(config, s));
    L2Z_CHECK(s->sh.hs <= 256, L2Z_ERR_INVALID, "%s: head_size above 256", fn);
    VerifyDraw store;
    const VerifyDraw *draw = nullptr;
    L2Z_TRY(verify_sample_args(temperature, top_p, coins, &store, &draw));
    if (draw != nullptr)  // one coin per depth
        for (int d = 0; d <= max_depth; d++)
            L2Z_CHECK(coins[d] >= 0.0f && coins[d] < 1.0f, L2Z_ERR_INVALID, "%s: coins[%d] = %g outside [0, 1)", fn, d,
                      (double)coins[d]);
    L2Z_CHECK(pos0 >= 0 && pos0 <= config->seq_len - n, L2Z_ERR_STATE, "%s: cache rows %d .. %lld outside [0, %d)", fn, pos0,
              (long long)pos0 + n - 1, config->seq_len);
    for (int i = 0; i < n; i++)
        L2Z_CHECK(tokens[i] >= 0 && tokens[i] < config->vocab_size, L2Z_ERR_STATE, "%s: tokens[%d] = %d out of vocabulary", fn,
                  i, tokens[i]);
    L2Z_HIP(hipSetDevice(s->device));
    L2Z_TRY(batch_alloc(s));
    L2Z_TRY(verify_alloc(s));
    if (draw != nullptr) L2Z_TRY(sample_alloc(s));
    BatchScratch *b = s->bt;
    const size_t hs = (size_t)config->dim / config->n_heads;
    BatchTable t = {};
    for (int i = 0; i < n; i++) {
        t.tokens[i] = tokens[i];
        t.pos[i] = pos0 + g.depth[i];  // RoPE and the cache index of the step's epilogue ...
        t.kc[i] = s->key_cache + (size_t)(i - g.depth[i]) * hs;  // ... which so lands in physical row pos0 + i (i >= depth)
        t.vc[i] = s->value_cache + (size_t)(i - g.depth[i]) * hs;
        t.logits[i] = b->v_logits + (size_t)i * config->vocab_size;
        if (draw != nullptr) {
            t.temperature[i] = draw->temperature;
            t.top_p[i] = draw->top_p;
            t.coin[i] = draw->coins[g.depth[i]];
        }
    }
    hipStream_t st = s->stream;
    L2Z_TRY(upload_tables(b, t, g, st));
    L2Z_TRY(batch_step(n, *config, s, w, b, pos0, 0, 0, max_depth));
    if (draw != nullptr) {
        SampleArgs a = {};
        a.tab = b->d_tab; a.scratch = b->smp; a.row_stride = b->smp_stride; a.vocab = config->vocab_size;
        a.out = b->d_vout;
        L2Z_HIP(launch_sample_batch(a, n, st));
    } else {
        L2Z_HIP(launch_verify_tree_argmax(b->v_logits, config->vocab_size, b->d_vout, n, st));
    }
    L2Z_HIP(launch_verify_tree_accept(b->d_tab, b->d_tree, b->v_logits, config->vocab_size, b->d_vout, s->logits, n, st));
    L2Z_HIP(launch_verify_tree_compact(s->key_cache, s->value_cache, b->d_vout, n, pos0, (int)hs, (size_t)config->seq_len * hs,
                                       config->n_layers, config->n_kv_heads, st));
    L2Z_HIP(hipMemcpyAsync(b->h_vout, b->d_vout, (size_t)(2 * n + 1) * 4, hipMemcpyDeviceToHost, st));
    b->v_rows = n;
    s->n_part = 0;  // l2z_argmax scans the logits the verdict copied
    s->logits_partial = false;
    return L2Z_OK;
}

}  // namespace
}  // namespace l2z

extern "C" int l2z_verify_tree(const int32_t *tokens, const int32_t *parent, int n_nodes, int pos0, float temperature,
                               float top_p, const float *coins, const l2z_config *config, l2z_runstate *s,
                               const l2z_weights *w, int32_t *out_next, int32_t *out_path, int *out_accepted)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out_next != nullptr && out_path != nullptr && out_accepted != nullptr, L2Z_ERR_INVALID,
              "l2z_verify_tree: null argument");
    L2Z_TRY(verify_tree_enqueue(tokens, parent, n_nodes, pos0, temperature, top_p, coins, config, s, w));
    BatchScratch *b = s->bt;
    L2Z_HIP(hipStreamSynchronize(s->stream));
    const int a = b->h_vout[n_nodes];
    memcpy(out_next, b->h_vout, (size_t)n_nodes * 4);
    memcpy(out_path, b->h_vout + n_nodes + 1, (size_t)(a + 1) * 4);
    *out_accepted = a;
    s->host_pos = pos0 + a + 1;
    return L2Z_OK;
}

// Testing support: l2z_verify_time for a tree (scripts/verify_tree_bench.py): one l2z_verify_tree call, then `iters` passes
// back to back (verdict, compaction and the copy included, no sync).  The passes rewrite the same KV rows; a pass whose
// verdict moved rows leaves the next one the same inputs, since every node's row is written again before it is read.
extern "C" int l2z_verify_tree_time(const int32_t *tokens, const int32_t *parent, int n_nodes, int pos0, float temperature,
                                    float top_p, const float *coins, const l2z_config *config, l2z_runstate *s,
                                    const l2z_weights *w, int iters, double *out_ms)
{
    L2Z_CHECK(iters >= 1 && out_ms != nullptr, L2Z_ERR_INVALID, "l2z_verify_tree_time: bad arguments");
    int32_t next[kBatchMax], path[kBatchMax];
    int acc = 0;
    L2Z_TRY(l2z_verify_tree(tokens, parent, n_nodes, pos0, temperature, top_p, coins, config, s, w, next, path, &acc));
    hipStream_t st = s->stream;
    hipEvent_t e0, e1;
    L2Z_HIP(hipEventCreate(&e0));
    L2Z_HIP(hipEventCreate(&e1));
    int rc = L2Z_OK;
    if (hipEventRecord(e0, st) != hipSuccess) rc = L2Z_ERR_HIP;
    for (int i = 0; i < iters && rc == L2Z_OK; i++)
        rc = verify_tree_enqueue(tokens, parent, n_nodes, pos0, temperature, top_p, coins, config, s, w);
    float ms = 0.0f;
    if (rc == L2Z_OK && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                         hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
        rc = L2Z_ERR_HIP;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc == L2Z_OK) *out_ms = ms / iters;
    return rc;
}

// Testing support (include/llama2_hip_test.h): row `row` of the last l2z_verify call's logits matrix
extern "C" int l2z_verify_logits_read(l2z_runstate *s, int row, float *out)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(s != nullptr && out != nullptr, L2Z_ERR_INVALID, "l2z_verify_logits_read: null argument");
    L2Z_CHECK(s->bt != nullptr && s->bt->v_logits != nullptr && row >= 0 && row < s->bt->v_rows, L2Z_ERR_STATE,
              "l2z_verify_logits_read: row %d is not a row of this runstate's last l2z_verify call", row);
    L2Z_HIP(hipSetDevice(s->device));
    L2Z_HIP(hipMemcpyAsync(out, s->bt->v_logits + (size_t)row * s->cfg.vocab_size, (size_t)s->cfg.vocab_size * 4,
                           hipMemcpyDeviceToHost, s->stream));
    L2Z_HIP(hipStreamSynchronize(s->stream));
    return L2Z_OK;
}

// Testing support: one l2z_verify call, then `iters` passes back to back (verdict and its copy included, no sync), timed
// by device events on the runstate's stream (scripts/verify_bench.py).  The passes rewrite the same KV rows.
extern "C" int l2z_verify_time(const int32_t *tokens, int n_tokens, int pos0, const l2z_config *config, l2z_runstate *s,
                               const l2z_weights *w, int iters, double *out_ms)
{
    L2Z_CHECK(iters >= 1 && out_ms != nullptr, L2Z_ERR_INVALID, "l2z_verify_time: bad arguments");
    int32_t next[kBatchMax];
    int acc = 0;
    L2Z_TRY(l2z_verify(tokens, n_tokens, pos0, config, s, w, next, &acc));  // validates, allocates
    hipStream_t st = s->stream;
    hipEvent_t e0, e1;
    L2Z_HIP(hipEventCreate(&e0));
    L2Z_HIP(hipEventCreate(&e1));
    int rc = L2Z_OK;
    if (hipEventRecord(e0, st) != hipSuccess) rc = L2Z_ERR_HIP;
    for (int i = 0; i < iters && rc == L2Z_OK; i++) rc = verify_enqueue("l2z_verify", tokens, n_tokens, pos0, config, s, w);
    float ms = 0.0f;
    if (rc == L2Z_OK && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                         hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
        rc = L2Z_ERR_HIP;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc == L2Z_OK) *out_ms = ms / iters;
    return rc;
}

// Testing support: l2z_verify_time for a sampled pass (scripts/verify_sample_bench.py): one l2z_verify_sample call, then
// `iters` passes back to back with the rows' draws, the accept scan and the copy included, no sync.
extern "C" int l2z_verify_sample_time(const int32_t *tokens, int n_tokens, int pos0, float temperature, float top_p,
                                      const float *coins, const l2z_config *config, l2z_runstate *s, const l2z_weights *w,
                                      int iters, double *out_ms)
{
    L2Z_CHECK(iters >= 1 && out_ms != nullptr, L2Z_ERR_INVALID, "l2z_verify_sample_time: bad arguments");
    int32_t next[kBatchMax];
    int acc = 0;
    L2Z_TRY(l2z_verify_sample(tokens, n_tokens, pos0, temperature, top_p, coins, config, s, w, next, &acc));
    VerifyDraw store;
    const VerifyDraw *draw = nullptr;
    L2Z_TRY(verify_sample_args(temperature, top_p, coins, &store, &draw));
    hipStream_t st = s->stream;
    hipEvent_t e0, e1;
    L2Z_HIP(hipEventCreate(&e0));
    L2Z_HIP(hipEventCreate(&e1));
    int rc = L2Z_OK;
    if (hipEventRecord(e0, st) != hipSuccess) rc = L2Z_ERR_HIP;
    for (int i = 0; i < iters && rc == L2Z_OK; i++)
        rc = verify_enqueue("l2z_verify_sample", tokens, n_tokens, pos0, config, s, w, draw);
    float ms = 0.0f;
    if (rc == L2Z_OK && (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                         hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
        rc = L2Z_ERR_HIP;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc == L2Z_OK) *out_ms = ms / iters;
    return rc;
}
