// batch_host.h -- what the host files of a call that names several runstates, or draws tokens, share (batch_host.cpp: the
// batched step and what stands around it; verify_host.cpp: the verify family; wide_host.cpp: the wide step and its run;
// prefill_batch_host.cpp, prefill_host.cpp, forward.cpp): the rules for the runstates and for the arguments of a draw, the
// front of a call of the ragged family made of them (check_ragged_call), the stream hand-overs, the scratch allocation and
// the batched step itself.
#pragma once
#include <initializer_list>

#include "batch_decode.h"
#include "l2z_state.h"

namespace l2z {

// Scratch of the batched step, owned by the runstate that is states[0] of a call (allocated on its first such call,
// freed with it): the activation rows of kBatchMax sequences, the attention scores, the device table and its pinned
// host twin, and the events that order the pass against the runstates' own streams.
struct BatchScratch {
    float *x = nullptr, *xn = nullptr, *q = nullptr, *att = nullptr, *h1 = nullptr, *scores = nullptr;
    int ld_xn = 0, ld_att = 0, ld_h1 = 0;
    BatchTable *d_tab = nullptr, *h_tab = nullptr;
    // what sits behind the table in the same allocations: l2z_verify_batch's VerifyGroupTable or l2z_verify_tree's
    // VerifyTreeTable
    void *d_behind = nullptr, *h_behind = nullptr;
    int *d_tokens_out = nullptr, *h_tokens_out = nullptr;
    hipEvent_t ev_in[kBatchMax] = {};
    hipEvent_t ev_done = nullptr;
    hipEvent_t ev_upload = nullptr;  // the last table copy: the pinned table may be rewritten once it has completed
    float *smp = nullptr;            // sample_alloc: kBatchMax rows of sample_scratch_floats(vocab)
    size_t smp_stride = 0;
    // verify_alloc: the [kBatchMax, vocab] logits matrix, the attention partials ([kBatchMax, n_heads, v_seg_cap,
    // head_size] and [..., 2]), the verdict on the device and pinned
    float *v_logits = nullptr, *v_part_o = nullptr, *v_part_ml = nullptr;
    int *d_vout = nullptr, *h_vout = nullptr;  // 3 * kBatchMax ints (l2z_verify: next[0 .. n) | accepted; l2z_verify_batch:
                                               // next[0 .. rows) | accepted[0 .. n); l2z_verify_tree: next[0 .. n) | accepted |
                                               // path[0 .. accepted])
    int v_seg_cap = 0, v_rows = 0;   // v_rows: rows of the last call (l2z_verify_logits_read)
    // q8_batch_alloc: the step's quantized rows on int8 group-quantized weights, [kBatchMax, max(dim, hidden_dim)] int8 and
    // their scales at group size q8_gs (a call with another group size re-makes them)
    int8_t *q8_xq = nullptr;
    float *q8_xs = nullptr;
    int q8_gs = 0;
};

// s->bt and what a call needs in it beyond the step's own: the sampler's scratch, the verify family's (each on first use)
int batch_alloc(l2z_runstate *s);
int sample_alloc(l2z_runstate *s);
int verify_alloc(l2z_runstate *s);
int q8_batch_alloc(l2z_runstate *s, int gs);

// What a call of the batched step on int8 group-quantized weights (l2z_transformer_batch_q8, l2z_verify_q8) asks beyond
// check_pair(..., q8_ok = true): such weights -- f32 and packed ones go to `f32_entry` --, and a shape the step's launches
// take; fn: the entry point a message names
int check_q8_step(const char *fn, const char *f32_entry, const l2z_runstate *s0, const l2z_weights *w);

// hipMalloc of every buffer of the list that has a size and is not there yet.  A failure leaves that pointer null, names
// `what` and the size in the error, and is L2Z_ERR_OOM where the device is out of memory; what was allocated before it
// stays with its owner, whose clean-up rule is the caller's.
struct DeviceBuf {
    void **p;
    size_t bytes;
};
int alloc_all(const char *what, std::initializer_list<DeviceBuf> want);

int no_device_check();
// the runstates of one call: non-null, pairwise distinct, unsharded, on one device, all made with *c (c: states[0]'s
// when the call names no config), 1 <= n <= n_max
int check_states(const char *fn, int n, l2z_runstate *const *states, const l2z_config *c, int n_max = kBatchMax);
// The preconditions of a call's rows; fn: the entry point a message names, where: "" or "sequence j: ".
// n rows from pos0 on lie in the cache; what: what the rows are to the caller
int check_positions(const char *fn, const char *where, const char *what, int pos0, int n, int seq_len);
// tokens[0 .. n) are in the vocabulary; a message names index first + i
int check_tokens(const char *fn, const char *where, const int32_t *tokens, int n, int vocab, int first = 0);
// row i of a call that takes a token and a position per runstate: its n_pos positions from pos on, then its token
int check_row(const char *fn, int i, int32_t token, int32_t pos, int n_pos, const l2z_config &c);
// l2z_sample_batch's rules for one temperature and top_p (seq >= 0: those of row or sequence seq) and the coins' presence ...
int check_draw(const char *fn, int seq, float temperature, float top_p, const float *coins);
// ... and for the `count` coins a sampled row reads, `stride` apart from coins[first] on
int check_coins(const char *fn, const float *coins, int first, int count, int stride = 1);

// A call of the ragged family (l2z_prefill_batch, l2z_transformer_wide, l2z_wide_run, l2z_verify_wide, l2z_step_mixed) as its
// arguments describe it: n sequences, one runstate each; sequence j brings n_tokens[j] rows (n_tokens null: one) at
// consecutive positions from pos0[j] on, the rows of all sequences behind one another in tokens; n_steps: the positions
// a sequence takes from its last row on (1; l2z_wide_run: its steps).
struct RaggedCall {
    const char *fn;          // the entry point a message names
    int n;
    const int32_t *tokens, *n_tokens, *pos0;
    int n_steps;
    // the draws: temperature null, none; else per sequence, and a sampled sequence's coins one per row (coins[row]), or --
    // coins_per_step -- one per step (coins[k * n + j])
    const float *temperature, *top_p, *coins;
    bool coins_per_step;
    const l2z_config *config;
    l2z_runstate *const *states;
    const l2z_weights *w;
    // the entry's limits: sequences, rows in all, rows of one sequence (0: as many as the cache holds)
    int max_seq, max_rows, max_seq_rows;
};
struct RaggedTotals {
    int R;          // rows in all
    int longest;    // rows of the longest sequence
    int deepest;    // the deepest position of a row
    bool sampled;   // some sequence draws
};
// The front of such a call; a refusal enqueues nothing and changes no state.  In this order: no device, null arguments, the
// runstates (check_states), one kind of cache (kv_check_kind), the row counts, every runstate against config and w
// (check_pair), states[0] on the prompt pass (prefill_check), the draws and their coins, then positions and tokens sequence
// by sequence.
int check_ragged_call(const RaggedCall &c, RaggedTotals *t);

// the pass on states[0]'s stream waits for everything already queued on every runstate's stream ... (b: a scratch with
// an event per runstate, ev_in[], and ev_done)
template <class Scratch> int join_streams(Scratch *b, int n, l2z_runstate *const *states)
{
    for (int i = 1; i < n; i++) {
        L2Z_HIP(hipEventRecord(b->ev_in[i], states[i]->stream));
        L2Z_HIP(hipStreamWaitEvent(states[0]->stream, b->ev_in[i], 0));
    }
    return L2Z_OK;
}
// ... and every runstate's stream waits for the pass
template <class Scratch> int release_streams(Scratch *b, int n, l2z_runstate *const *states)
{
    L2Z_HIP(hipEventRecord(b->ev_done, states[0]->stream));
    for (int i = 1; i < n; i++) L2Z_HIP(hipStreamWaitEvent(states[i]->stream, b->ev_done, 0));
    return L2Z_OK;
}

// The call left WHOLE logits in s, not a classifier's per-block candidates (l2z_argmax scans them), and s's next position
// is next_pos
inline void logits_whole(l2z_runstate *s, int next_pos)
{
    s->n_part = 0;
    s->logits_partial = false;
    s->host_pos = next_pos;
}

// the table of this call, and behind_bytes of what sits behind it, -> the device: one copy from the pinned buffer
// (rewritten only once the last copy is done)
int upload_table(BatchScratch *b, const BatchTable &t, hipStream_t st, const void *behind = nullptr, size_t behind_bytes = 0);

// A layer's attention as batch_step sees it: (layer_off) enqueues the launches that turn b->q into b->att for the layer
// whose caches start layer_off floats into each cache.
using LayerAttention = FnRef<int(size_t)>;

// The fields every attention form's args struct has, from the config and the step's scratch
template <class A> A attention_args(const l2z_config &c, const BatchScratch *b)
{
    A a = {};
    a.q = b->q; a.ldq = c.dim; a.out = b->att; a.ldo = b->ld_att;
    a.n_heads = c.n_heads; a.kv_mul = c.n_heads / c.n_kv_heads; a.head_size = c.dim / c.n_heads;
    a.kv_head_stride = (size_t)c.seq_len * a.head_size;
    return a;
}

// One step of the n rows of b->d_tab on s0's stream, each layer's attention by `attention`.  On int8 group-quantized
// weights (the caller has run q8_batch_alloc) it hands over to batch_step_q8 (q8_host.cpp), which walks
// the layers as the prompt pass on such weights does (q8_layers)
int batch_step(int n, const l2z_config &c, l2z_runstate *s0, const l2z_weights *w, BatchScratch *b, LayerAttention attention);
int batch_step_q8(int n, const l2z_config &c, l2z_runstate *s0, const l2z_weights *w, BatchScratch *b, LayerAttention attention);

// The rows' draws (l2z_sample_batch's launch) from tab->logits[i] with the table's temperature, top_p and coin -> out[0 .. n)
hipError_t sample_rows(BatchScratch *b, int vocab, int *out, int n, hipStream_t st);

// `iters` runs of pass() back to back on st between two device events -> *out_ms per run.  The events are destroyed on
// every path; the first error is returned.
int timed_loop(hipStream_t st, int iters, double *out_ms, FnRef<int()> pass);

}  // namespace l2z
