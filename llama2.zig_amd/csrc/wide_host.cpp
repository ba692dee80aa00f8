// wide_host.cpp -- host side of l2z_transformer_wide (include/llama2_hip_test.h): up to L2Z_WIDE_MAX independent sequences
// advanced by one token with one sweep of the weights.  The rows are ONE chunk of P = n rows of the ragged prompt pass
// (prefill_host.cpp) on states[0]'s prefill scratch and stream, so every product takes the whole model's form at that row
// count (short-prompt / panel / stream / tile, f32 or bf16 cores); what the step adds is the table with one sequence slot
// per row, the position-split decode attention and the launch that hands the [n, vocab] logits back (wide_decode.hip).
#include <cstring>

#include "batch_host.h"
#include "wide_decode.h"

static_assert(l2z::kWideMax == L2Z_WIDE_MAX, "include/llama2_hip_test.h L2Z_WIDE_MAX");

namespace l2z {

// Scratch of the wide step, owned by the runstate that is states[0] of a call (allocated on its first such call, freed
// with it): the key / value rows between their products and the scatter, the logits matrix, the attention partials, the
// rows' next ids, the device table with its pinned twin, and the events that order the pass against up to kWideMax
// streams (BatchScratch's are kBatchMax).
struct WideScratch {
    float *k = nullptr, *v = nullptr;   // [kWideMax, kv_dim]
    float *logits = nullptr;            // [kWideMax, ld_logits]
    int ld_logits = 0;                  // vocab_size rounded up to 4: every row 16-byte aligned
    float *part = nullptr;              // wide_part_floats
    int seg_cap = 0;
    int *d_next = nullptr, *h_next = nullptr;
    WideTable *d_tab = nullptr, *h_tab = nullptr;
    hipEvent_t ev_in[kWideMax] = {};
    hipEvent_t ev_done = nullptr;
    hipEvent_t ev_upload = nullptr;     // the last table copy: the pinned table may be rewritten once it has completed
};

void wide_free(l2z_runstate *s)
{
    WideScratch *b = s->wd;
    if (b == nullptr) return;
    void *ptrs[] = {b->k, b->v, b->logits, b->part, b->d_next, b->d_tab};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    if (b->h_next) (void)hipHostFree(b->h_next);
    if (b->h_tab) (void)hipHostFree(b->h_tab);
    for (hipEvent_t e : b->ev_in)
        if (e) (void)hipEventDestroy(e);
    if (b->ev_done) (void)hipEventDestroy(b->ev_done);
    if (b->ev_upload) (void)hipEventDestroy(b->ev_upload);
    delete b;
    s->wd = nullptr;
}

namespace {

int wide_alloc(l2z_runstate *s)
{
    if (s->wd != nullptr) return L2Z_OK;
    const l2z_config &c = s->cfg;
    WideScratch *b = new WideScratch();
    s->wd = b;
    const size_t R = kWideMax, kvd = (size_t)s->sh.kvd_loc;
    b->ld_logits = (c.vocab_size + 3) / 4 * 4;
    b->seg_cap = verify_segments(c.seq_len);
    struct { void **p; size_t bytes; } want[] = {
        {(void **)&b->k, R * kvd * 4}, {(void **)&b->v, R * kvd * 4}, {(void **)&b->logits, R * b->ld_logits * 4},
        {(void **)&b->part, wide_part_floats(c.n_heads, b->seg_cap, s->sh.hs) * 4},
        {(void **)&b->d_next, R * 4}, {(void **)&b->d_tab, sizeof(WideTable)}};
    for (auto &w : want) {
        const hipError_t e = hipMalloc(w.p, w.bytes);
        if (e != hipSuccess) {
            *w.p = nullptr;
            wide_free(s);  // the next call starts over
            set_error("l2z_transformer_wide scratch allocation (%zu bytes) failed: %s", w.bytes, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? L2Z_ERR_OOM : L2Z_ERR_HIP;
        }
    }
    int rc = L2Z_OK;
    auto hip = [&rc](hipError_t e) {
        if (rc == L2Z_OK && e != hipSuccess) {
            set_error("l2z_transformer_wide scratch: %s", hipGetErrorString(e));
            rc = L2Z_ERR_HIP;
        }
    };
    hip(hipHostMalloc((void **)&b->h_tab, sizeof(WideTable), hipHostMallocDefault));
    hip(hipHostMalloc((void **)&b->h_next, R * 4, hipHostMallocDefault));
    for (hipEvent_t &e : b->ev_in) hip(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hip(hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming));
    hip(hipEventCreateWithFlags(&b->ev_upload, hipEventDisableTiming));
    if (rc != L2Z_OK) wide_free(s);
    return rc;
}

}  // namespace
}  // namespace l2z

using namespace l2z;

extern "C" int l2z_transformer_wide(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                                    l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next)
{
    // ---- checks: a refusal enqueues nothing and changes no state ----
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && pos != nullptr && config != nullptr && w != nullptr, L2Z_ERR_INVALID,
              "l2z_transformer_wide: null argument");
    L2Z_TRY(check_states("l2z_transformer_wide", n, states, config, kWideMax));
    int deepest = 0;
    for (int i = 0; i < n; i++) {
        L2Z_TRY(check_pair(config, states[i], w));
        L2Z_CHECK(pos[i] >= 0 && pos[i] < config->seq_len, L2Z_ERR_STATE, "l2z_transformer_wide: pos[%d] = %d outside [0,%d)", i,
                  pos[i], config->seq_len);
        L2Z_CHECK(tokens[i] >= 0 && tokens[i] < config->vocab_size, L2Z_ERR_STATE,
                  "l2z_transformer_wide: tokens[%d] = %d out of vocabulary", i, tokens[i]);
        if (pos[i] > deepest) deepest = pos[i];
    }
    L2Z_TRY(prefill_check(config, states[0]));
    l2z_runstate *s0 = states[0];
    hipStream_t st = s0->stream;
    const l2z_config &c = *config;
    L2Z_HIP(hipSetDevice(s0->device));
    L2Z_TRY(prefill_scratch(s0, n));
    L2Z_TRY(wide_alloc(s0));
    WideScratch *b = s0->wd;

    // ---- the pass, on states[0]'s stream: it waits for every runstate's stream ... ----
    for (int i = 1; i < n; i++) {
        L2Z_HIP(hipEventRecord(b->ev_in[i], states[i]->stream));
        L2Z_HIP(hipStreamWaitEvent(st, b->ev_in[i], 0));
    }
    // the step's table, one copy from the pinned buffer (rewritten only once the last copy is done)
    L2Z_HIP(hipEventSynchronize(b->ev_upload));
    WideTable *t = b->h_tab;
    for (int i = 0; i < n; i++) {
        t->seq[i] = {states[i]->key_cache, states[i]->value_cache, i, 1, pos[i], 0};
        t->row_seq[i] = i;
        t->pos[i] = pos[i];
        t->tokens[i] = tokens[i];
        t->logits[i] = states[i]->logits;
    }
    L2Z_HIP(hipMemcpyAsync(b->d_tab, t, sizeof(WideTable), hipMemcpyHostToDevice, st));
    WideAttn wa = {b->d_tab, b->part, b->seg_cap, deepest / kVerifySeg + 1};
    RaggedChunk rg = {};
    rg.seq = b->d_tab->seq; rg.row_seq = b->d_tab->row_seq; rg.row_pos = b->d_tab->pos;
    rg.n_seq = n;
    rg.k = b->k; rg.v = b->v;
    rg.wide = &wa;
    // (the chunk's tokens go up from the pinned table too: the caller's array is free on return)
    L2Z_TRY(prefill_ragged_chunk(s0, w, t->tokens, n, rg));
    L2Z_HIP(hipEventRecord(b->ev_upload, st));
    L2Z_TRY(prefill_rows_logits(s0, w, n, b->logits, b->ld_logits));
    L2Z_HIP(launch_wide_logits_out(b->logits, b->ld_logits, b->d_tab, c.vocab_size, out_next ? b->d_next : nullptr, n, st));
    if (out_next) L2Z_HIP(hipMemcpyAsync(b->h_next, b->d_next, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    // ---- ... and every runstate's stream waits for the pass ----
    L2Z_HIP(hipEventRecord(b->ev_done, st));
    for (int i = 1; i < n; i++) L2Z_HIP(hipStreamWaitEvent(states[i]->stream, b->ev_done, 0));
    for (int i = 0; i < n; i++) {
        l2z_runstate *s = states[i];
        s->n_part = 0;  // l2z_argmax scans the logits: the classifier left no per-block candidates
        s->logits_partial = false;
        s->host_pos = pos[i] + 1;
    }
    if (out_next) {
        L2Z_HIP(hipStreamSynchronize(st));
        memcpy(out_next, b->h_next, (size_t)n * 4);
    }
    return L2Z_OK;
}
