// batch_host.h -- what the host files that run on the batched step share (batch_host.cpp: the step and what stands around
// it; verify_host.cpp: the verify family; prefill_batch_host.cpp: the rules of a call that names several runstates).
#pragma once
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
};

// s->bt and what a call needs in it beyond the step's own: the sampler's scratch, the verify family's (each on first use)
int batch_alloc(l2z_runstate *s);
int sample_alloc(l2z_runstate *s);
int verify_alloc(l2z_runstate *s);

int no_device_check();
// the runstates of one call: non-null, pairwise distinct, unsharded, on one device, all made with *c (c: states[0]'s
// when the call names no config), 1 <= n <= n_max
int check_states(const char *fn, int n, l2z_runstate *const *states, const l2z_config *c, int n_max = kBatchMax);
// the pass on states[0]'s stream waits for everything already queued on every runstate's stream ...
int join_streams(BatchScratch *b, int n, l2z_runstate *const *states);
// ... and every runstate's stream waits for the pass
int release_streams(BatchScratch *b, int n, l2z_runstate *const *states);

// the table of this call, and behind_bytes of what sits behind it, -> the device: one copy from the pinned buffer
// (rewritten only once the last copy is done)
int upload_table(BatchScratch *b, const BatchTable &t, hipStream_t st, const void *behind = nullptr, size_t behind_bytes = 0);

// A reference to a caller's callable (Args...) -> L2Z code, alive for the call it is passed to
template <class Sig> class FnRef;
template <class... Args> class FnRef<int(Args...)> {
  public:
    template <class F>
    FnRef(const F &f) : f_(&f), call_([](const void *p, Args... args) -> int { return (*(const F *)p)(args...); }) {}
    int operator()(Args... args) const { return call_(f_, args...); }

  private:
    const void *f_;
    int (*call_)(const void *, Args...);
};

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

// One step of the n rows of b->d_tab on s0's stream, each layer's attention by `attention`
int batch_step(int n, const l2z_config &c, l2z_runstate *s0, const l2z_weights *w, BatchScratch *b, LayerAttention attention);

// The rows' draws (l2z_sample_batch's launch) from tab->logits[i] with the table's temperature, top_p and coin -> out[0 .. n)
hipError_t sample_rows(BatchScratch *b, int vocab, int *out, int n, hipStream_t st);

// `iters` runs of pass() back to back on st between two device events -> *out_ms per run.  The events are destroyed on
// every path; the first error is returned.
int timed_loop(hipStream_t st, int iters, double *out_ms, FnRef<int()> pass);

}  // namespace l2z
