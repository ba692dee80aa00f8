// l2z_state.h -- the device-resident Weights / RunState objects behind the C ABI and the internal
// functions the translation units share (weights*.cpp, runstate.cpp, forward.cpp, prefill_host.cpp,
// hooks.cpp).  Product code; nothing under oracle/ is referenced.
#pragma once
#include <cstdint>
#include <vector>

#include "kv_pages.h"
#include "l2z_comm.h"
#include "l2z_internal.h"
#include "tunables.h"

namespace l2z {

struct BatchScratch;  // batch_host.h
struct WideScratch;   // wide_host.cpp

// ----- shard geometry (DESIGN.md "Sharding"; world == 1 -> everything local) -----
struct Shard {
    int rank = 0, world = 1;
    int hs = 0;        // head_size
    int dim0 = 0, dim_loc = 0;   // rows of q / wo / w2 and slice of x, xb owned here
    int kvd_loc = 0;             // local kv_dim (whole kv heads)
    int heads_loc = 0;
    int hid0 = 0, hid_loc = 0;   // rows of w1/w3, slice of hb
    int v0 = 0, v_loc = 0;       // rows of wcls, slice of logits
    // Scheme B (L2Z_SCHEME_B, world > 1): Wo and W2 are sharded by COLUMNS -- this rank holds the
    // columns its own heads / hidden rows feed, [dim][dimc_pad] and [dim][hidc_pad] per layer, the pad columns zero --
    // and produces a partial [dim] vector that an all-reduce sums.  dimc_pad / hidc_pad: dim_loc / hid_loc rounded
    // up to a width the vector mat-vec takes (pad_cols)
    bool scheme_b = false;
    int dimc_pad = 0, hidc_pad = 0;
};
int pad_cols(int n);  // widths above 768 floats: multiples of 256 (a row = whole 64-lane sweeps of 16 bytes); below: of 4
int make_shard(const l2z_config &c, const l2z_comm *comm, Shard *out);

// ----- the Weights.init pointer walk (main.zig:85-112) as a table -----
enum ShardKind { REPL, BY_Q_HEADS, BY_KV_HEADS, BY_HIDDEN, BY_DIM_ROWS, BY_VOCAB, SKIP };

struct TensorDesc {
    const char *name;
    size_t offset;  // f32 index in the file blob
    size_t layers, rows, cols;
    ShardKind kind;
    float scale, bias;  // synthetic generator
    size_t count() const { return layers * rows * cols; }
};
std::vector<TensorDesc> tensor_table(const l2z_config &c, bool shared);
void shard_rows(const TensorDesc &d, const Shard &s, size_t *r0, size_t *r1);

void build_packed(l2z_weights *w);  // weights_packed.cpp: the packed copy of a complete f32 weights object (best effort)

extern int g_cus;  // compute units of the device in use (set by ensure_device)
int ensure_device(int device);
int current_device_for(const l2z_comm *comm);

}  // namespace l2z

// the kinds of launch of the decode pass (l2z_time_kind, l2z_profile_forward; the packed copy and its mask are per kind)
enum { KIND_QKV = 0, KIND_ATTN, KIND_WO, KIND_FFN13, KIND_FFN2, KIND_CLS, KIND_ARGMAX, KIND_GATHER, KIND_COUNT };

struct l2z_weights {
    uint64_t uid = 0;  // unique per object for the life of the process: keys a runstate's captured graphs
    l2z_config cfg;
    int shared;
    int device;
    l2z::Shard sh;
    // one allocation: the tensors of the file in file order (this rank's rows of each), EXCEPT that W1 and W3
    // share one slot where W1 stood, row-interleaved -- [layer][row][W1 row | W3 row] -- so that the pair of rows
    // a feed-forward output needs is one contiguous run; W3's own slot is empty
    float *blob = nullptr;
    size_t blob_floats = 0;
    bool file_layout = false;    // world == 1: every tensor of the file is resident (the unread freq_cis tables too)
    std::vector<size_t> dev_off; // device offset (floats) of each tensor of the table; W3: that of the shared slot + cols
    // carved device pointers (local shards when world > 1)
    const float *tok_emb = nullptr, *rms_att = nullptr, *rms_ffn = nullptr, *rms_final = nullptr;
    const float *wq = nullptr, *wk = nullptr, *wv = nullptr, *wo = nullptr;
    // w1 / w3: row 0 of W1 / of W3 in the shared slot; consecutive rows of either are 2 * dim floats apart
    const float *w1 = nullptr, *w2 = nullptr, *w3 = nullptr, *wcls = nullptr;
    // the 29-bit packed copy of the decode's row mat-vec weights (packed_w.h; unsharded weights,
    // L2Z_PACKED_W), per kind of launch: ffn13 one W1 | W3 slot per layer, q|k|v three slots per layer (Wq, Wk, Wv, each
    // with its own base exponent), wo and ffn2 one per layer, cls one per model.  A kind has its own allocation (one that
    // fails costs that kind only); slots[i].p == null: that slot stays f32 only
    struct PkMat {
        const uint32_t *p = nullptr;
        int e = 0;          // base exponent E
        // the 28-bit form (pk28: rows of n == 4096 whose pairs have at most eight escapes; L2Z_PACKED_BITS): p is its
        // stream and rec the patch records, 16 dwords per pair; null: p is the 29-bit form
        const uint32_t *rec = nullptr;
        int bits() const { return p == nullptr ? 0 : rec != nullptr ? 28 : 29; }
        const float *src = nullptr;  // the f32 rows it stands for
        int rows = 0, cols = 0;
    };
    struct PkKind {
        uint32_t *blob = nullptr;
        std::vector<PkMat> slots;  // [layer][slot of the kind]
        int per_layer = 0;         // slots per layer (cls: 1, layer 0 only)
        int packed = 0;            // slots with a copy
    };
    PkKind pk[KIND_COUNT];
    // int8 group-quantized weights (l2z_weights_init_q8 / _q8_from): q8_gs != 0.  Such an object is
    // unsharded, has no f32 matrix and no packed slot -- blob is null and of the pointers above only rms_att, rms_ffn and
    // rms_final stand, inside q8_blob: one allocation of the three norm vectors and then, per tensor, its values
    // [layer][row][col] and its scales [layer][row][col / gs], W1 | W3 row-interleaved in one slot like the f32 layout.
    // Only the single-sequence decode and the q8 entry points of their own take it (check_pair's q8_ok)
    struct Q8Mat {
        const int8_t *q = nullptr;
        const float *s = nullptr;
    };
    int q8_gs = 0;
    uint8_t *q8_blob = nullptr;
    Q8Mat q_emb, q_wq, q_wk, q_wv, q_wo, q_w13, q_w2, q_cls;   // q_cls: q_emb's where the file shares them
    bool is_q8() const { return q8_gs != 0; }
    l2z::Q8Emb q8_emb() const { return l2z::Q8Emb{q_emb.q, q_emb.s, q8_gs}; }
    // slot j of `layer` of a kind, or null where the kind has no copy of it
    const PkMat *pk_slot(int kind, int layer, int j = 0) const
    {
        const PkKind &k = pk[kind];
        const size_t i = (size_t)layer * k.per_layer + j;
        return k.blob != nullptr && i < k.slots.size() && k.slots[i].p != nullptr ? &k.slots[i] : nullptr;
    }
};

// The KV page pool (include/llama2_hip_test.h; kv_pool.cpp): n_pages pages of the key array and as many of
// the value array, page p of either page_floats * p floats in, [layer][kv head][kKvPage][head_size]; zero-filled once
struct l2z_kvpool {
    l2z_config cfg;
    int device = 0;
    l2z::KvPages alloc;
    float *k = nullptr, *v = nullptr;
    size_t page_floats = 0;
    int live = 0;   // runstates made from it and not freed yet
};

static const char *const kKindNames[KIND_COUNT] = {"qkv", "attn", "wo", "ffn13", "ffn2", "cls", "argmax", "gather"};
static_assert(KIND_COUNT == L2Z_N_KINDS, "include/llama2_hip_test.h L2Z_N_KINDS");

struct l2z_runstate {
    l2z_config cfg;
    int device;
    l2z::Shard sh;
    const l2z_comm *comm = nullptr;
    hipStream_t stream = nullptr;
    // main.zig:119-135 (k, v, xb2, hb2, logits_indexed have no device twin:
    // k/v go straight into the cache rows, xb2/hb2 are fused away)
    float *x = nullptr, *xb = nullptr, *hb = nullptr, *q = nullptr, *logits = nullptr;
    float *part = nullptr;    // scheme B: this rank's partial [dim] output of wo / w2 (rank 0's includes the residual), summed by the all-reduce
    float *key_cache = nullptr, *value_cache = nullptr;   // (a paged runstate has neither)
    // l2z_runstate_init_paged: the pool the KV rows live in, this sequence's page table on the host, and its device
    // copy with the pinned twin the copy is made from (pages_dirty: the table changed since the last copy was enqueued)
    l2z_kvpool *pool = nullptr;
    l2z::KvSeq pg;
    int32_t *d_pages = nullptr, *h_pages = nullptr;
    bool pages_dirty = false;
    float2 *rope = nullptr;  // (seq_len, head_size/2) {cos, sin}
    // loop state on the device
    int *d_token = nullptr, *d_pos = nullptr, *d_prompt = nullptr, *d_n_prompt = nullptr;
    int *d_out_tokens = nullptr, *d_argmax = nullptr;
    // batched prefill scratch (allocated on first l2z_prefill): [kPrefillChunk, dim|hidden]
    float *pf_x = nullptr, *pf_xn = nullptr, *pf_q = nullptr, *pf_att = nullptr;
    float *pf_h1 = nullptr;
    int pf_ld_xn = 0, pf_ld_att = 0, pf_ld_h1 = 0;   // row pitches of pf_xn / pf_att / pf_h1 (prefill_host.cpp pf_ld: zero-padded)
    float *pf_stage = nullptr;  // sharded: [world][P, n_loc] blocks of the matrix being gathered
    float *pf_part = nullptr;   // scheme B: this rank's partial [P, dim] product of its column shard of Wo / W2
    int *pf_tokens = nullptr;
    l2z::DeferredSum pf_pending = {nullptr, 1, 128, 1, false};   // K ranges' sums of Wo / W2 the next rmsnorm launch adds (prefill_host.cpp)
    l2z::PlanesReady pf_planes_att = l2z::PLANES_SPLIT, pf_planes_h1 = l2z::PLANES_SPLIT;   // whether the attention output's / the gated rows' planes stand (prefill_host.cpp)
    l2z::SplitKWs pf_sk = {nullptr, nullptr, 0, 0, nullptr, 0, nullptr, 0};  // split-K workspace of the tile GEMM (chunks of <= 256 tokens)
    int pf_cap = 0;             // tokens per chunk the scratch above was allocated for
    // l2z_score (prefill_host.cpp; allocated on the first call, a runstate that never scores holds none of it):
    // sc_ws: one allocation per chunk capacity -- the [sc_cap, sc_slab_n] logits slab, the segments' partials, the targets' logits;
    // sc_seq: targets, log-probs and top-1 ids of a whole call (seq_len each), copied to the host once per call
    void *sc_ws = nullptr, *sc_seq = nullptr;
    size_t sc_ws_bytes = 0;
    int sc_cap = 0, sc_slab_n = 0;   // tokens per chunk / vocabulary columns per slab sc_ws was allocated for
    int sc_slab_force = 0;           // l2z_score_slab_set (tests): columns per slab, 0: by the workspace budget
    float *d_probs = nullptr;     // l2z_probs_read: softmax(logits / temperature), allocated on first use
    float *h_stage = nullptr;     // ... and its pinned host landing buffer
    // l2z_sample_run (allocated on the first call, a runstate that never samples in the loop holds none of it): what the
    // sampled step's last node reads -- {temperature, top_p}, then one coin per position (2 + seq_len floats) --, its pinned
    // host twin, and the row body's scratch (sample_scratch_floats(vocab))
    float *d_smp_ctl = nullptr, *h_smp_ctl = nullptr, *d_smp_scratch = nullptr;
    float *d_part_val = nullptr;  // classifier launch's per-block argmax candidates
    int *d_part_idx = nullptr;
    int n_part = 0;               // 0: argmax scans the logits instead
    int n_part_step = 0, n_part_fwd = 0;  // ... as left by the captured step / forward graphs (a shard's differ)
    float *d_attn_part = nullptr; // split attention: per (head, chunk) partials
    int *d_attn_cnt = nullptr;    // split attention: arrivals per local head (zero between launches)
    int attn_nch = 0;             // 0: one block per head at every position
    int attn_split_pos = 0;       // positions >= this use the split form (host picks the graph)
    int attn_short_pos = 0;       // positions < this use the 256-thread speculative one-block-per-head form
    int attn_split_wide_pos = 0;  // split form: 256 threads per block below this position, 1024 from it on
    // graphs, keyed by the uid of the weights they were captured with (a freed object's address
    // is commonly handed to the next one)
    uint64_t graph_w_uid = 0;
    hipGraphExec_t g_forward[4] = {nullptr, nullptr, nullptr, nullptr}, g_step[4] = {nullptr, nullptr, nullptr, nullptr};  // [attention variant]
    hipGraphExec_t g_sample[4] = {nullptr, nullptr, nullptr, nullptr};  // the sampled step's, each captured on its first sampled step (forward.cpp ensure_graph)
    bool use_graphs = true;
    int host_pos = 0;   // next position the greedy loop will run
    bool done = false;  // greedy loop saw BOS
    std::vector<int32_t> h_prompt;  // host copy of the greedy loop's prompt (prefill path)
    // peer-write transport: device copies of the four gathers' descriptions (xb, x, hb, logits) for
    // the kernels that push their outputs to the peers themselves (MatvecArgs::push)
    l2z::P2pArgs *d_push = nullptr;
    int n_gathers = 0;        // collectives per forward pass at world > 1: 4 gathers per layer + logits (scheme B: 2 all-reduces per layer + logits)
    bool ll_consume = false;  // peer-write transport, consumer side: mat-vecs read their gathered input
                              // as LL words from the landing slot; no gather launch except the logits
    // Greedy steps of a shard group on the peer-write transport end in a candidate exchange (ArgmaxArgs::xchg) instead
    // of the logits gather: after such a step `logits` holds only this rank's rows, and the first call that reads the
    // whole vector (l2z_logits_read, l2z_probs_read, l2z_argmax, l2z_runstate_read) gathers it -- a COLLECTIVE then:
    // every rank of the group makes it, as every rank makes every other call
    bool xchg_steps = false;
    bool logits_partial = false;
    bool fused_qkv_attn = false;  // small models: qkv + RoPE + KV write + attention in one launch
    int max_blocks = 0;
    bool packed_w = true;          // L2Z_PACKED_W at creation: decode mat-vecs stream the weights' packed copy where it exists
    int packed_kinds = -1;         // L2Z_PACKED_KINDS at creation: bit k = launches of kind k may take it
    int tl_attn_seq = 0;           // attention launches enqueued so far (AttnArgs::tl_seq, measurement builds)
    l2z::BatchScratch *bt = nullptr;  // batched decode scratch of the calls that name this runstate first (batch_host.cpp)
    // l2z_prefill_batch scratch of the calls that name this runstate first (prefill_batch_host.cpp): a chunk's key / value
    // rows [rg_cap, kv_dim] between their product and the scatter into the sequences' caches, and the chunk's table
    float *rg_k = nullptr, *rg_v = nullptr;
    void *rg_tab = nullptr;
    int rg_cap = 0;
    // l2z_prefill_q8 scratch (q8_host.cpp; allocated on the first call): one allocation, carved for chunks of up to
    // q8pf_cap rows at group size q8pf_gs
    void *q8pf = nullptr;
    int q8pf_cap = 0, q8pf_gs = 0;
    l2z::WideScratch *wd = nullptr;   // l2z_transformer_wide / l2z_wide_run scratch of the calls that name this runstate first (wide_host.cpp)
};

namespace l2z {

// forward.cpp
struct Prof;
// paged_ok: the entry point takes paged runstates (the wide family); every other one that touches a KV cache through
// s->key_cache refuses them here with L2Z_ERR_INVALID
// q8_ok: the entry point takes int8 group-quantized weights (the single-sequence decode: l2z_transformer, the greedy and
// sampled loops, l2z_time_kind, l2z_profile_forward); every other one refuses them here, before it enqueues anything
int check_pair(const l2z_config *config, const l2z_runstate *s, const l2z_weights *w, bool paged_ok = false,
               bool q8_ok = false);
// attention variant of a position (the host knows pos and replays the graph captured for its variant):
// 0 short context (256-thread speculative form), 1 one block per head as the shape picks, 2 split with 256
// threads per block, 3 split with 1024
enum { ATTN_SHORT = 0, ATTN_HEAD = 1, ATTN_SPLIT_S = 2, ATTN_SPLIT = 3, ATTN_VARIANTS = 4 };
// what follows the classifier in a pass: nothing (the logits are the result), the greedy loop's argmax + hand-over
// (argmax_kernel), or the sampled loop's draw + hand-over (sample_step_kernel; unsharded runstates, after l2z_sample_run
// has allocated what it reads)
enum StepKind { STEP_NONE = 0, STEP_GREEDY = 1, STEP_SAMPLE = 2 };
int enqueue_forward(l2z_runstate *s, const l2z_weights *w, StepKind step, Prof *prof, int only_stage,
                    int variant, int only_kind = -1);
int attn_variant(const l2z_runstate *s, int pos);
int run_forward(l2z_runstate *s, const l2z_weights *w, StepKind step, int pos);
int ensure_logits(l2z_runstate *s);  // gathers the logits if the last pass left only this rank's rows (see xchg_steps)
void drop_graphs(l2z_runstate *s);

// prefill_host.cpp
constexpr int kPrefillMinPrompt = L2Z_PREFILL_MIN_PROMPT;  // shorter prompts: the stepped loop is as fast
bool prefill_enabled();
bool prefill_usable(const l2z_runstate *s);
bool prefill_shard_takes_the_unsharded_kernels(const l2z_config &c, const Shard &sh);
int prefill_check(const l2z_config *config, const l2z_runstate *s);
struct ScoreCall;  // prefill_host.cpp: what an l2z_score call adds to every chunk of the pass (null: plain prefill)
int prefill_tokens(l2z_runstate *s, const l2z_weights *w, const int32_t *tokens, int n_tokens, int pos0,
                   const ScoreCall *score = nullptr);

// ... what l2z_prefill_batch shares with l2z_prefill (prefill_batch_host.cpp): the chunk scratch, one chunk's layers with
// the rows' sequences given by the table (every stage but q | k | v + attention is l2z_prefill's own), the classifier launch.
// tokens: the chunk's ids on the host, copied into pf_tokens first; null (l2z_wide_run from its second step on): they
// already stand in pf_tokens on the device, and the chunk makes no host-to-device copy
int prefill_scratch(l2z_runstate *s, int need);
int prefill_ragged_chunk(l2z_runstate *s, const l2z_weights *w, const int32_t *tokens, int P, const RaggedChunk &rg);
int prefill_last_logits(l2z_runstate *s, const l2z_weights *w);
// ... and with the wide and mixed calls (wide_host.cpp): the classifier over P rows of the chunk just run -- all of it, or
// the rows a device list names -- -> out [P, ldo]
int prefill_rows_logits(l2z_runstate *s, const l2z_weights *w, int P, float *out, int ldo, const int *rows = nullptr);
// prefill_batch_host.cpp: s's rg_k / rg_v (and l2z_prefill_batch's own table) for chunks of up to `need` rows
int ragged_alloc(l2z_runstate *s, int need);

// kv_pool.cpp: paged runstates in a call of the wide family (a call without them passes through all of these untouched)
// The runstates are of one kind -- all contiguous, or all paged from one pool made with their config --, else L2Z_ERR_INVALID
int kv_check_kind(const char *fn, int n, l2z_runstate *const *states);
// Before anything is enqueued: sequence j will write positions pos0[j] .. pos0[j] + (counts ? counts[j] : count) - 1.
// L2Z_ERR_STATE if one of them lies in a page shared with another sequence or a page below pos0[j] is not attached, L2Z_ERR_OOM if the pool's free pages do not cover
// what is missing -- nothing attached, nothing changed --, else every page is attached
int kv_attach(const char *fn, int n, l2z_runstate *const *states, const int32_t *pos0, const int32_t *counts, int count);
// the page tables that changed -> the device, on st (the pass's stream, after it has joined the runstates' streams)
int kv_upload(int n, l2z_runstate *const *states, hipStream_t st);
// s's entry of a RaggedSeq table: the caches, or the pool's arrays and the page table
void kv_seq_base(const l2z_runstate *s, RaggedSeq *q);
inline size_t kv_page_floats(const l2z_runstate *s) { return s->pool != nullptr ? s->pool->page_floats : 0; }
// s gives back every page wholly at or above n_pos, after its own stream has drained (every pass that read s's pages made
// that stream wait for it)
int kv_release(l2z_runstate *s, int n_pos);
// rows 0 .. n_pos - 1 of src's caches -> dst's, on dst's stream, either of them paged (both paged: rows r0 .. only)
int kv_copy_rows(l2z_runstate *dst, const l2z_runstate *src, int r0, int n_pos);
void kv_runstate_free(l2z_runstate *s);   // l2z_runstate_free's part: pages back, tables freed, the pool's count down

// batch_host.cpp
void batch_free(l2z_runstate *s);
// wide_host.cpp
void wide_free(l2z_runstate *s);
// l2z_verify_logits_read: row `row` of the logits matrix of s's last l2z_verify_wide call as states[0] (null: s's last verify
// call was not that, or the matrix has no such row); and the end of that: another call has taken the matrix or s's turn
const float *wide_verify_row(const l2z_runstate *s, int row);
void wide_verify_forget(l2z_runstate *s);

}  // namespace l2z
