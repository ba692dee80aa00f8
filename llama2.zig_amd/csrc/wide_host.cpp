// wide_host.cpp -- host side of l2z_transformer_wide, l2z_wide_run, l2z_verify_wide and l2z_step_mixed
// (include/llama2_hip_test.h): up to L2Z_WIDE_MAX independent sequences advanced by one token with one sweep of the weights,
// the loop of such steps kept on the device, the verify pass over up to L2Z_WIDE_MAX rows of many sequences, and the chunk
// that holds decode rows AND prompt rows.
// The rows are ONE chunk of the ragged prompt pass (prefill_host.cpp) on states[0]'s prefill scratch and stream, so every
// product takes the whole model's form at that row count (short-prompt / panel / stream / tile, f32 or bf16 cores).  The
// pass knows none of these calls: each hands it a RaggedChunk made from its device table (table_chunk) and the layers'
// attention as a callable bound to its own launcher and table -- the position-split decode attention (wide_decode.hip), the
// verify form whose block slots are ONE sequence's rows (wide_verify.hip), or the mixed dispatch (mixed_step.hip).
// Every entry point reads the same way: its arguments as a RaggedCall, the shared front (batch_host.h check_ragged_call)
// plus the refusals only it has, the frame's begin (wide_begin: scratch, pages, streams), its table (table_fill plus its
// own extras), its chunk, the classifier (all rows; l2z_step_mixed: the last rows only) and its last launch -- the one that
// hands the logits back, draws and advances inside a run (wide_sample.hip), gives the verdict, or draws and hands out --,
// its copy back, and the frame's end (wide_end).
#include <algorithm>
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

// the sampler's row body's scratch for kWideMax rows (a call in which some sequence draws)
int sampler_alloc(l2z_runstate *s)
{
    return alloc_all("wide sampler scratch", {{(void **)&s->wd->smp, (size_t)kWideMax * sample_scratch_floats(s->cfg.vocab_size) * 4}});
}

// what an l2z_wide_run call of `entries` = n_steps * n ids needs beyond the step's own
int run_alloc(l2z_runstate *s, size_t entries)
{
    WideScratch *b = s->wd;
    if (entries <= b->run_cap) return L2Z_OK;
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
    return L2Z_OK;
}

// l2z_step_mixed's own table, and the chunk's key / value rows before the scatter (WideScratch's hold kWideMax rows only)
int mixed_alloc(l2z_runstate *s, int R)
{
    WideScratch *b = s->wd;
    L2Z_TRY(ragged_alloc(s, R));
    if (b->d_mtab != nullptr && b->h_mtab != nullptr) return L2Z_OK;
    L2Z_TRY(alloc_all("l2z_step_mixed table", {{(void **)&b->d_mtab, sizeof(MixedTable)}}));
    if (b->h_mtab == nullptr) L2Z_HIP(hipHostMalloc((void **)&b->h_mtab, sizeof(MixedTable), hipHostMallocDefault));
    return L2Z_OK;
}

// ---- the frame of a pass: every entry point here is its RaggedCall, the front (check_ragged_call), wide_begin, its own table,
// its chunk(s) and last launch, its copy back, wide_end ----

// What stands between the front and the first launch, on states[0]: its device, the scratch of a chunk of t.R rows and of the
// wide step, the sampler's where some sequence draws, `more` (the entry's own allocations), the pages of paged runstates --
// the last refusal --, then the pass's stream joined with every runstate's and the page tables on their way.
// (A failure after join_streams returns without release_streams: the other runstates' streams are then not ordered behind
// what was enqueued.  "A refusal changes no state" covers the checks.)
int wide_begin(const RaggedCall &c, const RaggedTotals &t, FnRef<int()> more)
{
    l2z_runstate *s0 = c.states[0];
    L2Z_HIP(hipSetDevice(s0->device));
    L2Z_TRY(prefill_scratch(s0, t.R));
    L2Z_TRY(wide_alloc(s0));
    if (t.sampled) L2Z_TRY(sampler_alloc(s0));
    L2Z_TRY(more());
    L2Z_TRY(kv_attach(c.fn, c.n, c.states, c.pos0, c.n_tokens, c.n_tokens != nullptr ? 0 : c.n_steps));
    L2Z_TRY(join_streams(s0->wd, c.n, c.states));
    return kv_upload(c.n, c.states, s0->stream);
}
const auto nothing_more = []() -> int { return L2Z_OK; };   // (an entry with no allocations of its own)

// Every runstate's stream waits for the pass, and the host bookkeeping: states[0]'s matrix is this call's now, and a
// runstate's next position is the one behind its rows and steps (verdict_pending, l2z_verify_wide: known only once the
// verdict is back; what l2z_verify_logits_read may read is states[0]'s matrix and nothing older)
int wide_end(const RaggedCall &c, bool verdict_pending = false)
{
    L2Z_TRY(release_streams(c.states[0]->wd, c.n, c.states));
    for (int j = 0; j < c.n; j++) {
        l2z_runstate *s = c.states[j];
        if (!verdict_pending) logits_whole(s, c.pos0[j] + (c.n_tokens != nullptr ? c.n_tokens[j] : 1) + c.n_steps - 1);
        else if (s->bt != nullptr) s->bt->v_rows = 0;
        wide_verify_forget(s);
    }
    return L2Z_OK;
}

// The arrays both tables start with, filled from the call (t: the pinned twin): slot j = sequence j -- its caches or pages,
// its rows' place in the chunk, its runstate's logits -- and every row's slot, position and token
template <class Table> void table_fill(Table *t, const RaggedCall &c, int R)
{
    for (int j = 0, r = 0; j < c.n; j++) {
        const int rows = c.n_tokens != nullptr ? c.n_tokens[j] : 1;
        t->seq[j] = {nullptr, nullptr, r, rows, c.pos0[j], 0, nullptr};
        kv_seq_base(c.states[j], &t->seq[j]);
        t->logits[j] = c.states[j]->logits;
        for (int k = 0; k < rows; k++, r++) {
            t->row_seq[r] = j;
            t->pos[r] = c.pos0[j] + k;
        }
    }
    memcpy(t->tokens, c.tokens, (size_t)R * 4);
}

// ... and the chunk of the ragged pass that reads them on the device (d: the device table, of seq_max slots)
template <class Table> RaggedChunk table_chunk(const Table *d, int n_seq, int seq_max, float *k, float *v, const l2z_runstate *s0)
{
    RaggedChunk rg = {};
    rg.seq = d->seq; rg.row_seq = d->row_seq; rg.row_pos = d->pos;
    rg.n_seq = n_seq; rg.seq_max = seq_max;
    rg.k = k; rg.v = v;
    rg.page_floats = kv_page_floats(s0);
    return rg;
}

// the table of a step (a run: of its first step), one copy from the pinned buffer (rewritten only once the last copy is
// done).  sampled (l2z_verify_wide): the sequences' controls and the rows' coins go up behind the table in the same copy (a
// greedy sequence's coins are not read: 0 in their place).
int wide_upload_table(WideScratch *b, const RaggedCall &c, const RaggedTotals &tot)
{
    L2Z_HIP(hipEventSynchronize(b->ev_upload));
    WideTable *t = b->h_tab;
    table_fill(t, c, tot.R);
    const bool ctl_up = tot.sampled && !c.coins_per_step;
    if (ctl_up) {
        WideVerdictCtl *ctl = (WideVerdictCtl *)(t + 1);
        for (int j = 0; j < c.n; j++) {
            ctl->temperature[j] = c.temperature[j];
            ctl->top_p[j] = c.top_p[j];
            for (int r = t->seq[j].row0; r < t->seq[j].row0 + t->seq[j].rows; r++)
                ctl->coins[r] = c.temperature[j] > 0.0f ? c.coins[r] : 0.0f;
        }
    }
    L2Z_HIP(hipMemcpyAsync(b->d_tab, t, ctl_up ? kTabBytes : sizeof(WideTable), hipMemcpyHostToDevice, c.states[0]->stream));
    return L2Z_OK;
}

// The launches of ONE step of R rows of n_seq sequences on s0's stream, the same for every entry point: the rows as one
// chunk of the ragged prompt pass driven by the device table, the layers' attention the wide step's (verify_m == 0, a row
// per sequence) or l2z_verify_wide's (verify_m: the slots of an attention block); deepest: the step's deepest position, the
// attention grid's segment extent.  Then the classifier over all rows into b->logits, then the step's last launch.
// from_table: the rows' ids go up from the pinned table (the caller's array is free on return); otherwise they stand in
// pf_tokens, written by the step before.
int wide_step(l2z_runstate *s0, const l2z_weights *w, int n_seq, int R, int deepest, int verify_m, bool from_table, FnRef<int()> last)
{
    WideScratch *b = s0->wd;
    const WideAttn wa = {b->d_tab, b->part, b->seg_cap, deepest / kVerifySeg + 1, verify_m, n_seq, kv_page_floats(s0)};
    const auto layer = [&wa](const RaggedLayer &L, bool *planes_written) {
        return wa.verify_m != 0 ? launch_wide_verify_attention(L, wa, planes_written) : launch_wide_attention(L, wa, planes_written);
    };
    const RaggedAttention attention = layer;
    RaggedChunk rg = table_chunk(b->d_tab, n_seq, kWideMax, b->k, b->v, s0);
    rg.attention = &attention;
    L2Z_TRY(prefill_ragged_chunk(s0, w, from_table ? b->h_tab->tokens : nullptr, R, rg));
    if (from_table) L2Z_HIP(hipEventRecord(b->ev_upload, s0->stream));
    L2Z_TRY(prefill_rows_logits(s0, w, R, b->logits, b->ld_logits));
    return last();
}

}  // namespace
}  // namespace l2z

using namespace l2z;

extern "C" int l2z_transformer_wide(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                                    l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next)
{
    const RaggedCall call = {"l2z_transformer_wide", n, tokens, nullptr, pos, 1, nullptr, nullptr, nullptr, false,
                             config, states, w, kWideMax, 0, 0};
    RaggedTotals t;
    L2Z_TRY(check_ragged_call(call, &t));
    L2Z_TRY(wide_begin(call, t, nothing_more));
    l2z_runstate *s0 = states[0];
    WideScratch *b = s0->wd;
    hipStream_t st = s0->stream;
    L2Z_TRY(wide_upload_table(b, call, t));
    L2Z_TRY(wide_step(s0, w, n, n, t.deepest, 0, true, [&]() -> int {
        L2Z_HIP(launch_wide_logits_out(b->logits, b->ld_logits, b->d_tab, config->vocab_size, out_next ? b->d_next : nullptr, n, st));
        return L2Z_OK;
    }));
    if (out_next) L2Z_HIP(hipMemcpyAsync(b->h_next, b->d_next, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(wide_end(call));
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
    L2Z_TRY(no_device_check());
    L2Z_CHECK(out_tokens != nullptr, L2Z_ERR_INVALID, "l2z_wide_run: null argument");
    L2Z_CHECK(n_steps >= 1, L2Z_ERR_INVALID, "l2z_wide_run: n_steps = %d", n_steps);
    // (a row's coin of every step: coins[k * n + i])
    const RaggedCall call = {"l2z_wide_run", n, first_tokens, nullptr, pos0, n_steps, temperature, top_p, coins, true,
                             config, states, w, kWideMax, 0, 0};
    RaggedTotals t;
    L2Z_TRY(check_ragged_call(call, &t));
    const size_t entries = (size_t)n_steps * n;
    L2Z_TRY(wide_begin(call, t, [&]() { return run_alloc(states[0], entries); }));   // (paged runstates: every step's pages, up front)
    l2z_runstate *s0 = states[0];
    WideScratch *b = s0->wd;
    hipStream_t st = s0->stream;

    // ---- the run: the first step's table and the coins, n_steps steps back to back ----
    L2Z_TRY(wide_upload_table(b, call, t));
    WideDraw d = {};
    d.logits = b->logits; d.ld = b->ld_logits; d.vocab = config->vocab_size;
    d.tab = b->d_tab;
    d.tokens = s0->pf_tokens;
    if (t.sampled) {  // (the pinned twin is free: the run before has completed)
        memcpy(b->h_ctl, temperature, (size_t)n * 4);
        memcpy(b->h_ctl + kWideMax, top_p, (size_t)n * 4);
        memcpy(b->h_ctl + 2 * kWideMax, coins, entries * 4);
        L2Z_HIP(hipMemcpyAsync(b->d_ctl, b->h_ctl, (2 * (size_t)kWideMax + entries) * 4, hipMemcpyHostToDevice, st));
        d.temperature = b->d_ctl; d.top_p = b->d_ctl + kWideMax;
        d.scratch = b->smp; d.row_stride = sample_scratch_floats(config->vocab_size);
    }
    for (int k = 0; k < n_steps; k++) {
        // the step's own launches: its grids take the step's own deepest position, as the single call computes it
        if (t.sampled) d.coins = b->d_ctl + 2 * kWideMax + (size_t)k * n;
        d.ids = b->d_ids + (size_t)k * n;
        d.logits_out = k == n_steps - 1;
        L2Z_TRY(wide_step(s0, w, n, n, t.deepest + k, 0, k == 0, [&]() -> int {
            L2Z_HIP(launch_wide_draw_advance(d, n, st));
            return L2Z_OK;
        }));
    }
    L2Z_HIP(hipMemcpyAsync(b->h_ids, b->d_ids, entries * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(wide_end(call));
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_tokens, b->h_ids, entries * 4);
    return L2Z_OK;
}

// ---- l2z_verify_wide: the verify pass for up to kWideMax rows of many sequences in one sweep (include/llama2_hip_test.h) ----
extern "C" int l2z_verify_wide(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                               const float *temperature, const float *top_p, const float *coins, const l2z_config *config,
                               l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next, int32_t *out_accepted)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(n_tokens != nullptr && out_next != nullptr && out_accepted != nullptr, L2Z_ERR_INVALID, "l2z_verify_wide: null argument");
    const RaggedCall call = {"l2z_verify_wide", n, tokens, n_tokens, pos0, 1, temperature, top_p, coins, false,
                             config, states, w, kWideMax, kWideMax, kBatchMax};
    RaggedTotals t;
    L2Z_TRY(check_ragged_call(call, &t));
    L2Z_TRY(wide_begin(call, t, nothing_more));
    l2z_runstate *s0 = states[0];
    WideScratch *b = s0->wd;
    hipStream_t st = s0->stream;
    const int R = t.R;
    int m = 1;  // the smallest instantiation that holds the longest sequence
    while (m < t.longest) m <<= 1;

    // ---- the table (a slot per sequence, its rows behind one another), the chunk of R rows, the classifier over all of
    // them, the verdict, one copy back ----
    L2Z_TRY(wide_upload_table(b, call, t));
    WideVerdict d = {};
    d.logits = b->logits; d.ld = b->ld_logits; d.vocab = config->vocab_size;
    d.tab = b->d_tab;
    d.next = b->d_next; d.accepted = b->d_next + R;
    if (t.sampled) {
        d.ctl = (const WideVerdictCtl *)(b->d_tab + 1);
        d.scratch = b->smp; d.row_stride = sample_scratch_floats(config->vocab_size);
    }
    L2Z_TRY(wide_step(s0, w, n, R, t.deepest, m, true, [&]() -> int {
        L2Z_HIP(launch_wide_verdict(d, n, R, st));
        return L2Z_OK;
    }));
    L2Z_HIP(hipMemcpyAsync(b->h_next, b->d_next, (size_t)(R + n) * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(wide_end(call, true));
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
extern "C" int l2z_step_mixed(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                              const float *temperature, const float *top_p, const float *coins, const l2z_config *config,
                              l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next)
{
    L2Z_TRY(no_device_check());
    L2Z_CHECK(n_tokens != nullptr && out_next != nullptr, L2Z_ERR_INVALID, "l2z_step_mixed: null argument");
    // (a sequence draws once, from its last row: coins[j])
    const RaggedCall call = {"l2z_step_mixed", n, tokens, n_tokens, pos0, 1, temperature, top_p, coins, true,
                             config, states, w, kWideMax, kMixedRowsMax, 0};
    RaggedTotals t;
    L2Z_TRY(check_ragged_call(call, &t));
    const int R = t.R;
    MixedPlan plan;
    L2Z_CHECK(mixed_plan(n, n_tokens, pos0, &plan) && plan.R == R, L2Z_ERR_INVALID, "l2z_step_mixed: no plan for this layout");
    L2Z_TRY(wide_begin(call, t, [&]() { return mixed_alloc(states[0], R); }));
    l2z_runstate *s0 = states[0];
    WideScratch *b = s0->wd;
    hipStream_t st = s0->stream;

    // ---- the table (rewritten only once the last copy is done): what both tables start with, then the plan's lists and the
    // sequences' controls (a greedy sequence's coin is not read), one copy ----
    L2Z_HIP(hipEventSynchronize(b->ev_upload));
    MixedTable *mt = b->h_mtab;
    table_fill(mt, call, R);
    for (int j = 0; j < n; j++) {
        mt->last_row[j] = plan.last_row[j];
        mt->temperature[j] = t.sampled ? temperature[j] : 0.0f;
        mt->top_p[j] = t.sampled ? top_p[j] : 0.0f;
        mt->coins[j] = t.sampled && temperature[j] > 0.0f ? coins[j] : 0.0f;
    }
    memcpy(mt->prompt_rows, plan.prompt_rows, (size_t)plan.n_prompt_rows * 4);
    for (int i = 0; i < plan.n_dec; i++) mt->dec[i] = make_int2(plan.dec_row[i], plan.dec_seq[i]);
    for (int i = 0; i < plan.n_tiles; i++) mt->tiles[i] = make_int2(plan.tile_seq[i], plan.tile_q0[i]);
    L2Z_HIP(hipMemcpyAsync(b->d_mtab, mt, sizeof(MixedTable), hipMemcpyHostToDevice, st));

    // ---- ONE chunk of R rows: prompt attention for the sequences of several rows, the wide step's decode attention through
    // the (row, slot) list for the rest (mixed_step.hip) ----
    const MixedAttn ma = {b->d_mtab, b->part, b->seg_cap, std::max(plan.deepest_dec, 0) / kVerifySeg + 1, plan.n_dec,
                          plan.n_prompt_rows, kv_page_floats(s0)};
    RaggedChunk rg = table_chunk(b->d_mtab, n, kMixedSeqMax, s0->rg_k, s0->rg_v, s0);
    rg.tiles = b->d_mtab->tiles; rg.n_tiles = plan.n_tiles;
    rg.att_rows = b->d_mtab->prompt_rows; rg.n_att_rows = plan.n_prompt_rows;
    const auto layer = [&](const RaggedLayer &L, bool *planes_written) { return launch_mixed_attention(L, ma, rg, planes_written); };
    const RaggedAttention attention = layer;
    rg.attention = &attention;
    L2Z_TRY(prefill_ragged_chunk(s0, w, mt->tokens, R, rg));
    L2Z_HIP(hipEventRecord(b->ev_upload, st));
    // the classifier on the n LAST rows only: gathered and normed into a compact [n, dim] matrix, the product at n rows;
    // then the draw and the hand-out, one copy back
    L2Z_TRY(prefill_rows_logits(s0, w, n, b->logits, b->ld_logits, b->d_mtab->last_row));
    MixedDraw d = {};
    d.logits = b->logits; d.ld = b->ld_logits; d.vocab = config->vocab_size;
    d.tab = b->d_mtab;
    d.sampled = t.sampled;
    d.next = b->d_next;
    if (t.sampled) { d.scratch = b->smp; d.row_stride = sample_scratch_floats(config->vocab_size); }
    L2Z_HIP(launch_mixed_draw_out(d, n, st));
    L2Z_HIP(hipMemcpyAsync(b->h_next, b->d_next, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(wide_end(call));
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_next, b->h_next, (size_t)n * 4);
    return L2Z_OK;
}
