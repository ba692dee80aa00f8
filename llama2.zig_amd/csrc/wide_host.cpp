// wide_host.cpp -- host side of l2z_transformer_wide, l2z_wide_run and l2z_verify_wide (include/llama2_hip_test.h): up to
// L2Z_WIDE_MAX independent sequences advanced by one token with one sweep of the weights, the loop of such steps kept on the
// device, and the verify pass over up to L2Z_WIDE_MAX rows of many sequences.
// The rows are ONE chunk of P = n rows of the ragged prompt pass (prefill_host.cpp) on states[0]'s prefill scratch and
// stream, so every product takes the whole model's form at that row count (short-prompt / panel / stream / tile, f32 or
// bf16 cores); what the step adds is the table with one sequence slot per row, the position-split decode attention and its
// last launch: the one that hands the [n, vocab] logits back (wide_decode.hip), or, inside a run, the one that draws every
// row's token and hands the row to the next step (wide_sample.hip).  l2z_verify_wide is the same chunk with sequences of
// several rows: the table's slots are sequences, the attention takes a sequence's rows as a block's slots, and the last
// launches are the verdict (wide_verify.hip).  l2z_step_mixed (at the end of the file) is the chunk with sequences of one row
// AND sequences of many, up to kMixedRowsMax rows: its own table (mixed_plan.h, mixed_step.h), prompt attention for the
// multi-row sequences and the wide step's decode attention through a (row, slot) list for the rest, the classifier on the
// last rows only.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "batch_host.h"
#include "mixed_step.h"
#include "wide_decode.h"

static_assert(l2z::kWideMax == L2Z_WIDE_MAX, "include/llama2_hip_test.h L2Z_WIDE_MAX");
static_assert(l2z::kMixedSeqMax == L2Z_WIDE_MAX && l2z::kMixedRowsMax == L2Z_MIXED_ROWS_MAX, "include/llama2_hip_test.h L2Z_MIXED_ROWS_MAX");

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
    int *d_next = nullptr, *h_next = nullptr;   // [2 kWideMax]: the rows' ids; l2z_verify_wide: next[0 .. R) | accepted[0 .. n)
    WideTable *d_tab = nullptr, *h_tab = nullptr;   // with room for l2z_verify_wide's WideVerdictCtl behind
    int v_rows = 0;                     // rows of the logits matrix l2z_verify_logits_read may read: the last call was l2z_verify_wide
    hipEvent_t ev_in[kWideMax] = {};
    hipEvent_t ev_done = nullptr;
    hipEvent_t ev_upload = nullptr;     // the last table copy: the pinned table may be rewritten once it has completed
    // l2z_wide_run (each on the first call that needs it): a call's temperature | top_p ([kWideMax] each) | coins and its
    // ids, [n_steps, n] both, on the device and pinned, sized on demand; the sampler's scratch of kWideMax rows
    float *d_ctl = nullptr, *h_ctl = nullptr;
    int *d_ids = nullptr, *h_ids = nullptr;
    size_t run_cap = 0;                 // entries of coins / ids the four buffers hold
    float *smp = nullptr;               // kWideMax rows of sample_scratch_floats(vocab)
    // l2z_step_mixed (on the first such call): its own table, kMixedSeqMax sequences and kMixedRowsMax rows, and the pinned twin
    MixedTable *d_mtab = nullptr, *h_mtab = nullptr;
};

void wide_free(l2z_runstate *s)
{
    WideScratch *b = s->wd;
    if (b == nullptr) return;
    void *ptrs[] = {b->k, b->v, b->logits, b->part, b->d_next, b->d_tab, b->d_ctl, b->d_ids, b->smp, b->d_mtab};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    void *pinned[] = {b->h_next, b->h_tab, b->h_ctl, b->h_ids, b->h_mtab};
    for (void *p : pinned)
        if (p) (void)hipHostFree(p);
    for (hipEvent_t e : b->ev_in)
        if (e) (void)hipEventDestroy(e);
    if (b->ev_done) (void)hipEventDestroy(b->ev_done);
    if (b->ev_upload) (void)hipEventDestroy(b->ev_upload);
    delete b;
    s->wd = nullptr;
}

const float *wide_verify_row(const l2z_runstate *s, int row)
{
    const WideScratch *b = s->wd;
    return b != nullptr && row >= 0 && row < b->v_rows ? b->logits + (size_t)row * b->ld_logits : nullptr;
}

void wide_verify_forget(l2z_runstate *s)
{
    if (s->wd != nullptr) s->wd->v_rows = 0;
}

namespace {

constexpr size_t kTabBytes = sizeof(WideTable) + sizeof(WideVerdictCtl);
static_assert(sizeof(WideTable) % alignof(WideVerdictCtl) == 0, "the controls sit right behind the table");

int wide_alloc(l2z_runstate *s)
{
    if (s->wd != nullptr) return L2Z_OK;
    const l2z_config &c = s->cfg;
    WideScratch *b = new WideScratch();
    s->wd = b;
    const size_t R = kWideMax, kvd = (size_t)s->sh.kvd_loc;
    b->ld_logits = (c.vocab_size + 3) / 4 * 4;
    b->seg_cap = verify_segments(c.seq_len);
    int rc = alloc_all("l2z_transformer_wide scratch",
                       {{(void **)&b->k, R * kvd * 4}, {(void **)&b->v, R * kvd * 4}, {(void **)&b->logits, R * b->ld_logits * 4},
                        {(void **)&b->part, wide_part_floats(c.n_heads, b->seg_cap, s->sh.hs) * 4},
                        {(void **)&b->d_next, 2 * R * 4}, {(void **)&b->d_tab, kTabBytes}});
    auto hip = [&rc](hipError_t e) {
        if (rc == L2Z_OK && e != hipSuccess) {
            set_error("l2z_transformer_wide scratch: %s", hipGetErrorString(e));
            rc = L2Z_ERR_HIP;
        }
    };
    hip(hipHostMalloc((void **)&b->h_tab, kTabBytes, hipHostMallocDefault));
    hip(hipHostMalloc((void **)&b->h_next, 2 * R * 4, hipHostMallocDefault));
    for (hipEvent_t &e : b->ev_in) hip(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hip(hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming));
    hip(hipEventCreateWithFlags(&b->ev_upload, hipEventDisableTiming));
    if (rc != L2Z_OK) wide_free(s);  // the next call starts over
    return rc;
}

// what an l2z_wide_run call of `entries` = n_steps * n ids needs beyond the step's own; sampled: the row body's scratch too
int run_alloc(l2z_runstate *s, size_t entries, bool sampled)
{
    WideScratch *b = s->wd;
    if (entries > b->run_cap) {
        // (every earlier run has completed: the call is synchronous)
        if (b->d_ctl) (void)hipFree(b->d_ctl);
        if (b->d_ids) (void)hipFree(b->d_ids);
        if (b->h_ctl) (void)hipHostFree(b->h_ctl);
        if (b->h_ids) (void)hipHostFree(b->h_ids);
        b->d_ctl = b->h_ctl = nullptr;
        b->d_ids = b->h_ids = nullptr;
        b->run_cap = 0;
        const size_t cap = (entries + 4095) / 4096 * 4096, ctl = (2 * (size_t)kWideMax + cap) * 4;
        hipError_t e = hipMalloc((void **)&b->d_ctl, ctl);
        if (e == hipSuccess) e = hipMalloc((void **)&b->d_ids, cap * 4);
        if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_ctl, ctl, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_ids, cap * 4, hipHostMallocDefault);
        if (e != hipSuccess) {  // (what was allocated is freed on the next attempt)
            set_error("l2z_wide_run coins / ids allocation (%zu bytes) failed: %s", ctl + cap * 4, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? L2Z_ERR_OOM : L2Z_ERR_HIP;
        }
        b->run_cap = cap;
    }
    if (sampled)
        L2Z_TRY(alloc_all("l2z_wide_run sampler scratch",
                          {{(void **)&b->smp, (size_t)kWideMax * sample_scratch_floats(s->cfg.vocab_size) * 4}}));
    return L2Z_OK;
}

// The checks both entry points share: the runstates, the weights, and every row's first token and its positions
// pos[i] .. pos[i] + n_steps - 1.  *deepest: the deepest first position.
int wide_checks(const char *fn, int n, const int32_t *tokens, const int32_t *pos, int n_steps, const l2z_config *config,
                l2z_runstate *const *states, const l2z_weights *w, int *deepest)
{
    L2Z_CHECK(tokens != nullptr && pos != nullptr && config != nullptr && w != nullptr, L2Z_ERR_INVALID, "%s: null argument", fn);
    L2Z_TRY(check_states(fn, n, states, config, kWideMax));
    L2Z_TRY(kv_check_kind(fn, n, states));
    *deepest = 0;
    for (int i = 0; i < n; i++) {
        L2Z_TRY(check_pair(config, states[i], w, true));
        L2Z_TRY(check_row(fn, i, tokens[i], pos[i], n_steps, *config));
        if (pos[i] > *deepest) *deepest = pos[i];
    }
    return prefill_check(config, states[0]);
}

// every runstate's stream waits for the pass; the host bookkeeping of a runstate whose next position is pos[i] + steps
int wide_release(WideScratch *b, int n, l2z_runstate *const *states, const int32_t *pos, int steps)
{
    L2Z_TRY(release_streams(b, n, states));
    for (int i = 0; i < n; i++) {
        logits_whole(states[i], pos[i] + steps);
        wide_verify_forget(states[i]);  // (states[0]'s matrix is this call's now)
    }
    return L2Z_OK;
}

// the table of a step (a run: of its first step), one copy from the pinned buffer (rewritten only once the last copy is done).
// n_tokens == null: a row per sequence, at pos[i].  l2z_verify_wide: sequence i's n_tokens[i] rows stand behind one another
// from pos[i] on, tokens is per row, and, temperature != null, the sequences' controls and the rows' coins go up behind the
// table in the same copy (a greedy sequence's coins are not read: 0 in their place).
int wide_upload_table(WideScratch *b, int n, const int32_t *tokens, const int32_t *pos, l2z_runstate *const *states,
                      const int32_t *n_tokens = nullptr, const float *temperature = nullptr, const float *top_p = nullptr,
                      const float *coins = nullptr)
{
    L2Z_HIP(hipEventSynchronize(b->ev_upload));
    WideTable *t = b->h_tab;
    WideVerdictCtl *ctl = (WideVerdictCtl *)(t + 1);
    for (int i = 0, r = 0; i < n; i++) {
        const int rows = n_tokens ? n_tokens[i] : 1;
        t->seq[i] = {nullptr, nullptr, r, rows, pos[i], 0, nullptr};
        kv_seq_base(states[i], &t->seq[i]);
        t->logits[i] = states[i]->logits;
        if (temperature) {
            ctl->temperature[i] = temperature[i];
            ctl->top_p[i] = top_p[i];
        }
        for (int k = 0; k < rows; k++, r++) {
            t->row_seq[r] = i;
            t->pos[r] = pos[i] + k;
            t->tokens[r] = tokens[r];
            if (temperature) ctl->coins[r] = temperature[i] > 0.0f ? coins[r] : 0.0f;
        }
    }
    L2Z_HIP(hipMemcpyAsync(b->d_tab, t, temperature ? kTabBytes : sizeof(WideTable), hipMemcpyHostToDevice, states[0]->stream));
    return L2Z_OK;
}

// The launches of ONE step of n rows on s0's stream, the same for every entry point: the rows as one chunk of the ragged
// prompt pass driven by the device table (deepest: the step's deepest position, the attention grid's segment extent),
// the classifier over all rows into b->logits, then the step's last launch.  from_table: the rows' ids go up from the
// pinned table (the caller's array is free on return); otherwise they stand in pf_tokens, written by the step before.
// n_seq, verify_m: the step's own are n and 0, a sequence per row; l2z_verify_wide's are its sequences and the slots of
// an attention block.
int wide_step(l2z_runstate *s0, const l2z_weights *w, int n, int deepest, bool from_table, FnRef<int()> last, int n_seq = 0,
              int verify_m = 0)
{
    WideScratch *b = s0->wd;
    WideAttn wa = {b->d_tab, b->part, b->seg_cap, deepest / kVerifySeg + 1, verify_m, kv_page_floats(s0)};
    RaggedChunk rg = {};
    rg.seq = b->d_tab->seq; rg.row_seq = b->d_tab->row_seq; rg.row_pos = b->d_tab->pos;
    rg.n_seq = verify_m ? n_seq : n;
    rg.k = b->k; rg.v = b->v;
    rg.page_floats = wa.page_floats;
    rg.wide = &wa;
    L2Z_TRY(prefill_ragged_chunk(s0, w, from_table ? b->h_tab->tokens : nullptr, n, rg));
    if (from_table) L2Z_HIP(hipEventRecord(b->ev_upload, s0->stream));
    L2Z_TRY(prefill_rows_logits(s0, w, n, b->logits, b->ld_logits));
    return last();
}

}  // namespace
}  // namespace l2z

using namespace l2z;

extern "C" int l2z_transformer_wide(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                                    l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next)
{
    // ---- checks: a refusal enqueues nothing and changes no state ----
    L2Z_TRY(no_device_check());
    int deepest = 0;
    L2Z_TRY(wide_checks("l2z_transformer_wide", n, tokens, pos, 1, config, states, w, &deepest));
    l2z_runstate *s0 = states[0];
    hipStream_t st = s0->stream;
    L2Z_HIP(hipSetDevice(s0->device));
    L2Z_TRY(prefill_scratch(s0, n));
    L2Z_TRY(wide_alloc(s0));
    WideScratch *b = s0->wd;
    L2Z_TRY(kv_attach("l2z_transformer_wide", n, states, pos, nullptr, 1));   // (paged runstates: the last refusal)

    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(kv_upload(n, states, st));
    L2Z_TRY(wide_upload_table(b, n, tokens, pos, states));
    L2Z_TRY(wide_step(s0, w, n, deepest, true, [&]() -> int {
        L2Z_HIP(launch_wide_logits_out(b->logits, b->ld_logits, b->d_tab, config->vocab_size, out_next ? b->d_next : nullptr, n, st));
        return L2Z_OK;
    }));
    if (out_next) L2Z_HIP(hipMemcpyAsync(b->h_next, b->d_next, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(wide_release(b, n, states, pos, 1));
    if (out_next) {
        L2Z_HIP(hipStreamSynchronize(st));
        memcpy(out_next, b->h_next, (size_t)n * 4);
    }
    return L2Z_OK;
}

extern "C" int l2z_wide_run(int n, const int32_t *first_tokens, const int32_t *pos0, int n_steps, const float *temperature,
                            const float *top_p, const float *coins, const l2z_config *config, l2z_runstate *const *states,
                            const l2z_weights *w, int32_t *out_tokens)
{
    // ---- checks: a refusal enqueues nothing and changes no state ----
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out_tokens != nullptr, L2Z_ERR_INVALID, "l2z_wide_run: null argument");
    L2Z_CHECK(n_steps >= 1, L2Z_ERR_INVALID, "l2z_wide_run: n_steps = %d", n_steps);
    int deepest = 0;
    L2Z_TRY(wide_checks("l2z_wide_run", n, first_tokens, pos0, n_steps, config, states, w, &deepest));
    bool sampled = false;  // some row draws: l2z_sample_batch's rules for it
    if (temperature != nullptr) {
        L2Z_CHECK(top_p != nullptr, L2Z_ERR_INVALID, "l2z_wide_run: top_p is NULL beside temperature");
        for (int i = 0; i < n; i++) {
            L2Z_TRY(check_draw("l2z_wide_run", i, temperature[i], top_p[i], coins));
            if (temperature[i] == 0.0f) continue;
            sampled = true;
            L2Z_TRY(check_coins("l2z_wide_run", coins, i, n_steps, n));  // the row's coin of every step: coins[k * n + i]
        }
    }
    l2z_runstate *s0 = states[0];
    hipStream_t st = s0->stream;
    const size_t entries = (size_t)n_steps * n;
    L2Z_HIP(hipSetDevice(s0->device));
    L2Z_TRY(prefill_scratch(s0, n));
    L2Z_TRY(wide_alloc(s0));
    L2Z_TRY(run_alloc(s0, entries, sampled));
    WideScratch *b = s0->wd;
    L2Z_TRY(kv_attach("l2z_wide_run", n, states, pos0, nullptr, n_steps));   // (paged runstates: every step's pages, up front)

    // ---- the run, on states[0]'s stream: one join, the first step's table and the coins, n_steps steps back to back ----
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(kv_upload(n, states, st));
    L2Z_TRY(wide_upload_table(b, n, first_tokens, pos0, states));
    WideDraw d = {};
    d.logits = b->logits; d.ld = b->ld_logits; d.vocab = config->vocab_size;
    d.tab = b->d_tab;
    d.tokens = s0->pf_tokens;
    if (sampled) {  // (the pinned twin is free: the run before has completed)
        memcpy(b->h_ctl, temperature, (size_t)n * 4);
        memcpy(b->h_ctl + kWideMax, top_p, (size_t)n * 4);
        memcpy(b->h_ctl + 2 * kWideMax, coins, entries * 4);
        L2Z_HIP(hipMemcpyAsync(b->d_ctl, b->h_ctl, (2 * (size_t)kWideMax + entries) * 4, hipMemcpyHostToDevice, st));
        d.temperature = b->d_ctl; d.top_p = b->d_ctl + kWideMax;
        d.scratch = b->smp; d.row_stride = sample_scratch_floats(config->vocab_size);
    }
    for (int k = 0; k < n_steps; k++) {
        // the step's own launches: its grids take the step's own deepest position, as the single call computes it
        if (sampled) d.coins = b->d_ctl + 2 * kWideMax + (size_t)k * n;
        d.ids = b->d_ids + (size_t)k * n;
        d.logits_out = k == n_steps - 1;
        L2Z_TRY(wide_step(s0, w, n, deepest + k, k == 0, [&]() -> int {
            L2Z_HIP(launch_wide_draw_advance(d, n, st));
            return L2Z_OK;
        }));
    }
    L2Z_HIP(hipMemcpyAsync(b->h_ids, b->d_ids, entries * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(wide_release(b, n, states, pos0, n_steps));
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_tokens, b->h_ids, entries * 4);
    return L2Z_OK;
}

// ---- l2z_verify_wide: the verify pass for up to kWideMax rows of many sequences in one sweep (include/llama2_hip_test.h) ----
extern "C" int l2z_verify_wide(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                               const float *temperature, const float *top_p, const float *coins, const l2z_config *config,
                               l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next, int32_t *out_accepted)
{
    const char *fn = "l2z_verify_wide";
    // ---- checks: a refusal enqueues nothing and changes no state (l2z_verify_batch's, with the wide limits) ----
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && n_tokens != nullptr && pos0 != nullptr && config != nullptr && w != nullptr &&
                  out_next != nullptr && out_accepted != nullptr,
              L2Z_ERR_INVALID, "%s: null argument", fn);
    L2Z_TRY(check_states(fn, n, states, config, kWideMax));
    L2Z_TRY(kv_check_kind(fn, n, states));
    int R = 0, longest = 0, deepest = 0;
    for (int j = 0; j < n; j++) {
        L2Z_CHECK(n_tokens[j] >= 1 && n_tokens[j] <= kBatchMax, L2Z_ERR_INVALID, "%s: n_tokens[%d] = %d outside [1, %d]", fn, j,
                  n_tokens[j], kBatchMax);
        R += n_tokens[j];
        longest = std::max(longest, n_tokens[j]);
    }
    L2Z_CHECK(R <= kWideMax, L2Z_ERR_INVALID, "%s: %d rows in all, above %d", fn, R, kWideMax);
    for (int j = 0; j < n; j++) L2Z_TRY(check_pair(config, states[j], w, true));
    L2Z_TRY(prefill_check(config, states[0]));
    L2Z_CHECK(states[0]->sh.hs <= 256, L2Z_ERR_INVALID, "%s: head_size above 256", fn);
    bool sampled = false;  // some sequence draws: l2z_sample_batch's rules for it
    if (temperature != nullptr) {
        L2Z_CHECK(top_p != nullptr, L2Z_ERR_INVALID, "%s: top_p is NULL beside a temperature array", fn);
        for (int j = 0, r = 0; j < n; r += n_tokens[j], j++) {
            L2Z_TRY(check_draw(fn, j, temperature[j], top_p[j], coins));
            if (temperature[j] == 0.0f) continue;
            sampled = true;
            L2Z_TRY(check_coins(fn, coins, r, n_tokens[j]));
        }
    }
    for (int j = 0, r = 0; j < n; r += n_tokens[j], j++) {
        char where[32];
        snprintf(where, sizeof where, "sequence %d: ", j);
        L2Z_TRY(check_positions(fn, where, "positions", pos0[j], n_tokens[j], config->seq_len));
        L2Z_TRY(check_tokens(fn, where, tokens + r, n_tokens[j], config->vocab_size));
        deepest = std::max(deepest, pos0[j] + n_tokens[j] - 1);
    }
    l2z_runstate *s0 = states[0];
    hipStream_t st = s0->stream;
    L2Z_HIP(hipSetDevice(s0->device));
    L2Z_TRY(prefill_scratch(s0, R));
    L2Z_TRY(wide_alloc(s0));
    WideScratch *b = s0->wd;
    if (sampled)
        L2Z_TRY(alloc_all("l2z_verify_wide sampler scratch",
                          {{(void **)&b->smp, (size_t)kWideMax * sample_scratch_floats(config->vocab_size) * 4}}));
    int m = 1;  // the smallest instantiation that holds the longest sequence
    while (m < longest) m <<= 1;
    L2Z_TRY(kv_attach(fn, n, states, pos0, n_tokens, 0));   // (paged runstates: the last refusal)

    // ---- the pass, on states[0]'s stream: the table (a slot per sequence, its rows behind one another), the chunk of R
    // rows, the classifier over all of them, the verdict, one copy back ----
    // (a failure from here on returns without release_streams, as in l2z_transformer_wide and l2z_wide_run: the other
    // runstates' streams are then not ordered behind what was enqueued.  "A refusal changes no state" covers the checks.)
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(kv_upload(n, states, st));
    L2Z_TRY(wide_upload_table(b, n, tokens, pos0, states, n_tokens, sampled ? temperature : nullptr, top_p, coins));
    WideVerdict d = {};
    d.logits = b->logits; d.ld = b->ld_logits; d.vocab = config->vocab_size;
    d.tab = b->d_tab;
    d.next = b->d_next; d.accepted = b->d_next + R;
    if (sampled) {
        d.ctl = (const WideVerdictCtl *)(b->d_tab + 1);
        d.scratch = b->smp; d.row_stride = sample_scratch_floats(config->vocab_size);
    }
    L2Z_TRY(wide_step(s0, w, R, deepest, true, [&]() -> int {
        L2Z_HIP(launch_wide_verdict(d, n, R, st));
        return L2Z_OK;
    }, n, m));
    L2Z_HIP(hipMemcpyAsync(b->h_next, b->d_next, (size_t)(R + n) * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(release_streams(b, n, states));
    for (int j = 0; j < n; j++) {  // the matrix is states[0]'s: l2z_verify_logits_read finds it there and nowhere else
        if (states[j]->bt != nullptr) states[j]->bt->v_rows = 0;
        wide_verify_forget(states[j]);
    }
    L2Z_HIP(hipStreamSynchronize(st));
    b->v_rows = R;  // (only a pass that completed leaves the hook a matrix)
    memcpy(out_next, b->h_next, (size_t)R * 4);
    for (int j = 0; j < n; j++) {
        out_accepted[j] = b->h_next[R + j];
        logits_whole(states[j], pos0[j] + out_accepted[j] + 1);
    }
    return L2Z_OK;
}

// ---- l2z_step_mixed: prompt chunks and decode rows in ONE chunk of the ragged prompt pass (include/llama2_hip_test.h) ----
namespace l2z {
namespace {

int mixed_alloc(l2z_runstate *s)
{
    WideScratch *b = s->wd;
    if (b->d_mtab != nullptr && b->h_mtab != nullptr) return L2Z_OK;
    L2Z_TRY(alloc_all("l2z_step_mixed table", {{(void **)&b->d_mtab, sizeof(MixedTable)}}));
    if (b->h_mtab == nullptr) L2Z_HIP(hipHostMalloc((void **)&b->h_mtab, sizeof(MixedTable), hipHostMallocDefault));
    return L2Z_OK;
}

// the plan and the call's arguments -> the pinned table (rewritten only once the last copy is done), one copy
int mixed_upload_table(WideScratch *b, const MixedPlan &p, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                       l2z_runstate *const *states, const float *temperature, const float *top_p, const float *coins)
{
    L2Z_HIP(hipEventSynchronize(b->ev_upload));
    MixedTable *t = b->h_mtab;
    for (int j = 0; j < p.n; j++) {
        t->seq[j] = {nullptr, nullptr, p.seq_row0[j], n_tokens[j], pos0[j], 0, nullptr};
        kv_seq_base(states[j], &t->seq[j]);
        t->logits[j] = states[j]->logits;
        t->last_row[j] = p.last_row[j];
        t->temperature[j] = temperature ? temperature[j] : 0.0f;
        t->top_p[j] = temperature ? top_p[j] : 0.0f;
        t->coins[j] = temperature && temperature[j] > 0.0f ? coins[j] : 0.0f;   // (a greedy sequence's coin is not read)
    }
    memcpy(t->row_seq, p.row_seq, (size_t)p.R * 4);
    memcpy(t->pos, p.row_pos, (size_t)p.R * 4);
    memcpy(t->tokens, tokens, (size_t)p.R * 4);
    memcpy(t->prompt_rows, p.prompt_rows, (size_t)p.n_prompt_rows * 4);
    for (int i = 0; i < p.n_dec; i++) t->dec[i] = make_int2(p.dec_row[i], p.dec_seq[i]);
    for (int i = 0; i < p.n_tiles; i++) t->tiles[i] = make_int2(p.tile_seq[i], p.tile_q0[i]);
    L2Z_HIP(hipMemcpyAsync(b->d_mtab, t, sizeof(MixedTable), hipMemcpyHostToDevice, states[0]->stream));
    return L2Z_OK;
}

}  // namespace
}  // namespace l2z

extern "C" int l2z_step_mixed(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                              const float *temperature, const float *top_p, const float *coins, const l2z_config *config,
                              l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next)
{
    const char *fn = "l2z_step_mixed";
    // ---- checks: a refusal enqueues nothing and changes no state (l2z_verify_wide's, with this call's limits) ----
    L2Z_TRY(no_device_check());
    L2Z_CHECK(tokens != nullptr && n_tokens != nullptr && pos0 != nullptr && config != nullptr && w != nullptr && out_next != nullptr,
              L2Z_ERR_INVALID, "%s: null argument", fn);
    L2Z_TRY(check_states(fn, n, states, config, kWideMax));
    L2Z_TRY(kv_check_kind(fn, n, states));
    long long rows = 0;
    for (int j = 0; j < n; j++) {
        L2Z_CHECK(n_tokens[j] >= 1, L2Z_ERR_INVALID, "%s: n_tokens[%d] = %d (at least 1)", fn, j, n_tokens[j]);
        rows += n_tokens[j];
        L2Z_CHECK(rows <= kMixedRowsMax, L2Z_ERR_INVALID, "%s: more than %d rows in all", fn, kMixedRowsMax);
    }
    const int R = (int)rows;
    for (int j = 0; j < n; j++) L2Z_TRY(check_pair(config, states[j], w, true));
    L2Z_TRY(prefill_check(config, states[0]));
    L2Z_CHECK(states[0]->sh.hs <= 256, L2Z_ERR_INVALID, "%s: head_size above 256", fn);
    bool sampled = false;  // some sequence draws: l2z_sample_batch's rules for it
    if (temperature != nullptr) {
        L2Z_CHECK(top_p != nullptr, L2Z_ERR_INVALID, "%s: top_p is NULL beside a temperature array", fn);
        for (int j = 0; j < n; j++) {
            L2Z_TRY(check_draw(fn, j, temperature[j], top_p[j], coins));
            if (temperature[j] == 0.0f) continue;
            sampled = true;
            L2Z_TRY(check_coins(fn, coins, j, 1));
        }
    }
    for (int j = 0, r = 0; j < n; r += n_tokens[j], j++) {
        char where[32];
        snprintf(where, sizeof where, "sequence %d: ", j);
        L2Z_TRY(check_positions(fn, where, "positions", pos0[j], n_tokens[j], config->seq_len));
        L2Z_TRY(check_tokens(fn, where, tokens + r, n_tokens[j], config->vocab_size));
    }
    MixedPlan plan;
    L2Z_CHECK(mixed_plan(n, n_tokens, pos0, &plan) && plan.R == R, L2Z_ERR_INVALID, "%s: no plan for this layout", fn);
    l2z_runstate *s0 = states[0];
    hipStream_t st = s0->stream;
    L2Z_HIP(hipSetDevice(s0->device));
    L2Z_TRY(prefill_scratch(s0, R));
    L2Z_TRY(ragged_alloc(s0, R));   // (the chunk's key / value rows before the scatter: WideScratch's hold kWideMax rows only)
    L2Z_TRY(wide_alloc(s0));
    L2Z_TRY(mixed_alloc(s0));
    WideScratch *b = s0->wd;
    if (sampled)
        L2Z_TRY(alloc_all("l2z_step_mixed sampler scratch",
                          {{(void **)&b->smp, (size_t)kWideMax * sample_scratch_floats(config->vocab_size) * 4}}));
    L2Z_TRY(kv_attach(fn, n, states, pos0, n_tokens, 0));   // (paged runstates: the last refusal)

    // ---- the pass, on states[0]'s stream: the table, ONE chunk of R rows, the classifier over the n last rows, the draw
    // and the hand-out, one copy back ----
    L2Z_TRY(join_streams(b, n, states));
    L2Z_TRY(kv_upload(n, states, st));
    L2Z_TRY(mixed_upload_table(b, plan, tokens, n_tokens, pos0, states, sampled ? temperature : nullptr, top_p, coins));
    MixedAttn ma = {b->d_mtab, b->part, b->seg_cap, std::max(plan.deepest_dec, 0) / kVerifySeg + 1, plan.n_dec,
                    plan.n_prompt_rows, kv_page_floats(s0)};
    RaggedChunk rg = {};
    rg.seq = b->d_mtab->seq; rg.row_seq = b->d_mtab->row_seq; rg.row_pos = b->d_mtab->pos;
    rg.tiles = b->d_mtab->tiles;
    rg.n_seq = n; rg.n_tiles = plan.n_tiles;
    rg.k = s0->rg_k; rg.v = s0->rg_v;
    rg.page_floats = ma.page_floats;
    rg.mixed = &ma;
    rg.att_rows = b->d_mtab->prompt_rows; rg.n_att_rows = plan.n_prompt_rows;
    L2Z_TRY(prefill_ragged_chunk(s0, w, b->h_mtab->tokens, R, rg));
    L2Z_HIP(hipEventRecord(b->ev_upload, st));
    // the classifier on the n LAST rows only: gathered and normed into a compact [n, dim] matrix, the product at n rows
    L2Z_TRY(prefill_rows_logits(s0, w, n, b->logits, b->ld_logits, b->d_mtab->last_row));
    MixedDraw d = {};
    d.logits = b->logits; d.ld = b->ld_logits; d.vocab = config->vocab_size;
    d.tab = b->d_mtab;
    d.sampled = sampled;
    d.next = b->d_next;
    if (sampled) { d.scratch = b->smp; d.row_stride = sample_scratch_floats(config->vocab_size); }
    L2Z_HIP(launch_mixed_draw_out(d, n, st));
    L2Z_HIP(hipMemcpyAsync(b->h_next, b->d_next, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(release_streams(b, n, states));
    for (int j = 0; j < n; j++) {
        logits_whole(states[j], pos0[j] + n_tokens[j]);
        wide_verify_forget(states[j]);  // (states[0]'s matrix is this call's now)
    }
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_next, b->h_next, (size_t)n * 4);
    return L2Z_OK;
}
