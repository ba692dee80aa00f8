// wide_host.cpp -- host side of l2z_transformer_wide, l2z_transformer_wide_q8, l2z_wide_run, l2z_verify_wide and l2z_step_mixed
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
#include "kv8.h"
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
    Owned<float> k, v;                  // [kWideMax, kv_dim]
    Owned<float> logits;                // [kWideMax, ld_logits]
    int ld_logits = 0;                  // vocab_size rounded up to 4: every row 16-byte aligned
    Owned<float> part;                  // wide_part_floats
    int seg_cap = 0;
    Owned<int> d_next;                  // [2 kWideMax]: the rows' ids; l2z_verify_wide: next[0 .. R) | accepted[0 .. n)
    Pinned<int> h_next;
    Owned<WideTable> d_tab;             // with room for l2z_verify_wide's WideVerdictCtl behind
    Pinned<WideTable> h_tab;
    int v_rows = 0;                     // rows of the logits matrix l2z_verify_logits_read may read: the last call was l2z_verify_wide
    OwnedEvent ev_in[kWideMax];
    OwnedEvent ev_done;
    OwnedEvent ev_upload;               // the last table copy: the pinned table may be rewritten once it has completed
    // l2z_wide_run (each on the first call that needs it): a call's temperature | top_p ([kWideMax] each) | coins and its
    // ids, [n_steps, n] both, on the device and pinned, sized on demand; the sampler's scratch of kWideMax rows
    Owned<float> d_ctl;
    Pinned<float> h_ctl;
    Owned<int> d_ids;
    Pinned<int> h_ids;
    int run_cap = 0;                    // entries of coins / ids the four buffers hold
    Owned<float> smp;                   // kWideMax rows of sample_scratch_floats(vocab)
    // l2z_step_mixed (on the first such call): its own table, kMixedSeqMax sequences and kMixedRowsMax rows, and the pinned
    // twin (mtab_cap: 0 or 1, both are there)
    Owned<MixedTable> d_mtab;
    Pinned<MixedTable> h_mtab;
    int mtab_cap = 0;
    // l2z_transformer_wide_q8 (on the first such call): the step's quantized rows, [kWideMax, max(dim, hidden_dim)] int8, and
    // their scales at group size q8_gs (a call with another group size re-makes them; q8_cap: 0 or 1, both are there)
    Owned<int8_t> q8_xq;
    Owned<float> q8_xs;
    int q8_cap = 0, q8_gs = 0;
};

void WideScratchDelete::operator()(WideScratch *b) const { delete b; }

const float *wide_verify_row(const l2z_runstate *s, int row)
{
    const WideScratch *b = s->wd.get();
    return b != nullptr && row >= 0 && row < b->v_rows ? b->logits + (size_t)row * b->ld_logits : nullptr;
}

void wide_verify_forget(l2z_runstate *s)
{
    if (s->wd != nullptr) s->wd->v_rows = 0;
}

namespace {

// behind the table, in the same allocations and the same copy: l2z_verify_wide's controls, or the sequences' int8 arrays
// (l2z_transformer_wide_q8 on runstates with int8 KV rows: Kv8Seq, slot j = sequence j)
constexpr size_t kCtlBytes = sizeof(WideTable) + sizeof(WideVerdictCtl), kKv8Bytes = sizeof(WideTable) + kWideMax * sizeof(Kv8Seq);
constexpr size_t kTabBytes = kCtlBytes > kKv8Bytes ? kCtlBytes : kKv8Bytes;
static_assert(sizeof(WideTable) % alignof(WideVerdictCtl) == 0, "the controls sit right behind the table");
static_assert(sizeof(WideTable) % alignof(Kv8Seq) == 0, "the int8 arrays' table sits right behind the table");

int wide_alloc(l2z_runstate *s)
{
    if (s->wd != nullptr) return L2Z_OK;
    const l2z_config &c = s->cfg;
    // built here, the runstate's only once all of it stands: a failure below frees what there is with `made`
    std::unique_ptr<WideScratch, WideScratchDelete> made(new WideScratch());
    WideScratch *b = made.get();
    const size_t R = kWideMax, kvd = (size_t)s->sh.kvd_loc;
    b->ld_logits = (c.vocab_size + 3) / 4 * 4;
    b->seg_cap = verify_segments(c.seq_len);
    int cap = 0;
    L2Z_TRY(grow("l2z_transformer_wide scratch", &cap, 1, 1, nullptr, 0, [] { return L2Z_OK; },
                 {{b->k, R * kvd * 4}, {b->v, R * kvd * 4}, {b->logits, R * b->ld_logits * 4},
                  {b->part, wide_part_floats(c.n_heads, b->seg_cap, s->sh.hs) * 4}, {b->d_next, 2 * R * 4}, {b->d_tab, kTabBytes},
                  {b->h_tab, kTabBytes}, {b->h_next, 2 * R * 4}}));
    for (OwnedEvent &e : b->ev_in) L2Z_HIP(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
    L2Z_HIP(hipEventCreateWithFlags(b->ev_done.put(), hipEventDisableTiming));
    L2Z_HIP(hipEventCreateWithFlags(b->ev_upload.put(), hipEventDisableTiming));
    s->wd = std::move(made);
    return L2Z_OK;
}

// the sampler's row body's scratch for kWideMax rows (a call in which some sequence draws)
int sampler_alloc(l2z_runstate *s)
{
    return s->wd->smp.make((size_t)kWideMax * sample_scratch_floats(s->cfg.vocab_size) * 4, "wide sampler scratch");
}

// what an l2z_wide_run call of `entries` = n_steps * n ids needs beyond the step's own
int run_alloc(l2z_runstate *s, int entries)
{
    WideScratch *b = s->wd.get();
    const size_t cap = (size_t)round_cap(entries, 4096), ctl = (2 * (size_t)kWideMax + cap) * 4;
    // (nothing to drain: every earlier run has completed, the call is synchronous)
    return grow("l2z_wide_run coins / ids", &b->run_cap, entries, 4096, nullptr, 0, [] { return L2Z_OK; },
                {{b->d_ctl, ctl}, {b->d_ids, cap * 4}, {b->h_ctl, ctl}, {b->h_ids, cap * 4}});
}

// l2z_step_mixed's own table, and the chunk's key / value rows before the scatter (WideScratch's hold kWideMax rows only)
int mixed_alloc(l2z_runstate *s, int R)
{
    WideScratch *b = s->wd.get();
    L2Z_TRY(ragged_alloc(s, R));
    return grow("l2z_step_mixed table", &b->mtab_cap, 1, 1, nullptr, 0, [] { return L2Z_OK; },
                {{b->d_mtab, sizeof(MixedTable)}, {b->h_mtab, sizeof(MixedTable)}});
}

// ---- the frame of a pass: every entry point here is its RaggedCall, the front (check_ragged_call), wide_begin, its own table,
// its chunk(s) and last launch, its copy back, wide_end ----

// What stands between the front and the first launch, on states[0]: its device, the scratch of a chunk of t.R rows and of the
// wide step, the sampler's where some sequence draws, `more` (the entry's own allocations), the pages of paged runstates --
// the last refusal --, then the pass's stream joined with every runstate's and the page tables on their way.
// pass: the scope of the pass, made here once the scratch with its events stands; wide_end releases it, and so does its
// end on every path that does not get there.  ("A refusal changes no state" covers the checks.)
int wide_begin(const RaggedCall &c, const RaggedTotals &t, FnRef<int()> more, std::optional<StreamScope> &pass)
{
    l2z_runstate *s0 = c.states[0];
    L2Z_HIP(hipSetDevice(s0->device));
    L2Z_TRY(prefill_scratch(s0, t.R));
    L2Z_TRY(wide_alloc(s0));
    if (t.sampled) L2Z_TRY(sampler_alloc(s0));
    L2Z_TRY(more());
    L2Z_TRY(kv_attach(c.fn, c.n, c.states, c.pos0, c.n_tokens, c.n_tokens != nullptr ? 0 : c.n_steps));
    pass.emplace(s0->wd.get(), c.n, c.states);
    L2Z_TRY(pass->joined());
    return kv_upload(c.n, c.states, s0->stream);
}
const auto nothing_more = []() -> int { return L2Z_OK; };   // (an entry with no allocations of its own)

// Every runstate's stream waits for the pass, and the host bookkeeping: states[0]'s matrix is this call's now, and a
// runstate's next position is the one behind its rows and steps (verdict_pending, l2z_verify_wide: known only once the
// verdict is back; what l2z_verify_logits_read may read is states[0]'s matrix and nothing older)
int wide_end(const RaggedCall &c, StreamScope &pass, bool verdict_pending = false)
{
    L2Z_TRY(pass.release());
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
    const bool kv8_up = c.states[0]->is_kv8();   // (never beside the controls: such runstates come to the q8 step alone)
    if (kv8_up) {
        Kv8Seq *q8 = (Kv8Seq *)(t + 1);
        for (int j = 0; j < c.n; j++) q8[j] = {c.states[j]->k8, c.states[j]->v8, c.states[j]->ks8, c.states[j]->vs8};
    }
    L2Z_HIP(hipMemcpyAsync(b->d_tab, t, ctl_up ? kCtlBytes : kv8_up ? kKv8Bytes : sizeof(WideTable), hipMemcpyHostToDevice,
                           c.states[0]->stream));
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
    WideScratch *b = s0->wd.get();
    const WideAttn wa = {b->d_tab, b->part, b->seg_cap, deepest / kVerifySeg + 1, verify_m, n_seq, kv_page_floats(s0)};
    const auto layer = [&wa](const RaggedLayer &L, bool *planes_written) {
        return wa.verify_m != 0 ? launch_wide_verify_attention(L, wa, planes_written) : launch_wide_attention(L, wa, planes_written);
    };
    const RaggedAttention attention = layer;
    RaggedChunk rg = table_chunk(b->d_tab.get(), n_seq, kWideMax, b->k, b->v, s0);
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
    std::optional<StreamScope> pass;
    L2Z_TRY(wide_begin(call, t, nothing_more, pass));
    l2z_runstate *s0 = states[0];
    WideScratch *b = s0->wd.get();
    hipStream_t st = s0->stream;
    L2Z_TRY(wide_upload_table(b, call, t));
    L2Z_TRY(wide_step(s0, w, n, n, t.deepest, 0, true, [&]() -> int {
        L2Z_HIP(launch_wide_logits_out(b->logits, b->ld_logits, b->d_tab, config->vocab_size, out_next ? b->d_next : nullptr, n, st));
        return L2Z_OK;
    }));
    if (out_next) L2Z_HIP(hipMemcpyAsync(b->h_next, b->d_next, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(wide_end(call, *pass));
    if (out_next) {
        L2Z_HIP(hipStreamSynchronize(st));
        memcpy(out_next, b->h_next, (size_t)n * 4);
    }
    return L2Z_OK;
}

// PREVIEW (include/llama2_hip_test.h): l2z_transformer_wide's contract on int8 group-quantized weights.  The
// frame is the wide family's; the step is wide_step_q8 (q8_host.cpp), the layers' attention the wide step's own.
extern "C" int l2z_transformer_wide_q8(int n, const int32_t *tokens, const int32_t *pos, const l2z_config *config,
                                       l2z_runstate *const *states, const l2z_weights *w, int32_t *out_next)
{
    const RaggedCall call = {"l2z_transformer_wide_q8", n, tokens, nullptr, pos, 1, nullptr, nullptr, nullptr, false,
                             config, states, w, kWideMax, 0, 0, true, "l2z_transformer_wide", true};
    RaggedTotals t;
    L2Z_TRY(check_ragged_call(call, &t));
    std::optional<StreamScope> pass;
    L2Z_TRY(wide_begin(call, t, [&]() { return q8_rows_alloc("l2z_transformer_wide_q8 scratch", states[0], states[0]->wd.get(), kWideMax, w->q8_gs); }, pass));
    l2z_runstate *s0 = states[0];
    WideScratch *b = s0->wd.get();
    hipStream_t st = s0->stream;
    L2Z_TRY(wide_upload_table(b, call, t));
    L2Z_HIP(hipEventRecord(b->ev_upload, st));
    const WideAttn wa = {b->d_tab, b->part, b->seg_cap, t.deepest / kVerifySeg + 1, 0, n, 0};
    // runstates with int8 KV rows (all of the call or none: kv_check_kind): the scatter and the attention of kv8.h over the
    // arrays' table behind the WideTable; else exactly the launches of the f32 caches
    const bool kv8 = s0->is_kv8();
    const Kv8Seq *seq8 = (const Kv8Seq *)(b->d_tab + 1);
    const auto layer = [&](const RaggedLayer &L, bool *planes_written) {
        return kv8 ? launch_kv8_attention(L, wa, seq8, planes_written) : launch_wide_attention(L, wa, planes_written);
    };
    const RaggedAttention attention = layer;
    RaggedChunk rg = table_chunk(b->d_tab.get(), n, kWideMax, b->k, b->v, s0);
    rg.attention = &attention;
    const auto scatter8 = [&](float *q, int ldq, int P, size_t layer_off, size_t kv_head_stride, hipStream_t stream) {
        return launch_kv8_rope_scatter(q, ldq, rg, seq8, P, config->dim, s0->sh.kvd_loc, s0->sh.hs, config->seq_len, s0->rope, layer_off,
                                       kv_head_stride, stream);
    };
    const RaggedScatter scatter = scatter8;
    if (kv8) rg.scatter = &scatter;
    L2Z_TRY(wide_step_q8(n, s0, w, rg, b->d_tab->tokens, b->q8_xq, b->q8_xs, b->logits, b->ld_logits));
    L2Z_HIP(launch_wide_logits_out(b->logits, b->ld_logits, b->d_tab, config->vocab_size, out_next ? b->d_next : nullptr, n, st));
    if (out_next) L2Z_HIP(hipMemcpyAsync(b->h_next, b->d_next, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    L2Z_TRY(wide_end(call, *pass));
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
    std::optional<StreamScope> pass;
    L2Z_TRY(wide_begin(call, t, [&]() { return run_alloc(states[0], (int)entries); }, pass));   // (paged runstates: every step's pages, up front)
    l2z_runstate *s0 = states[0];
    WideScratch *b = s0->wd.get();
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
    L2Z_TRY(wide_end(call, *pass));
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
    std::optional<StreamScope> pass;
    L2Z_TRY(wide_begin(call, t, nothing_more, pass));
    l2z_runstate *s0 = states[0];
    WideScratch *b = s0->wd.get();
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
    L2Z_TRY(wide_end(call, *pass, true));
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
    std::optional<StreamScope> pass;
    L2Z_TRY(wide_begin(call, t, [&]() { return mixed_alloc(states[0], R); }, pass));
    l2z_runstate *s0 = states[0];
    WideScratch *b = s0->wd.get();
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
    RaggedChunk rg = table_chunk(b->d_mtab.get(), n, kMixedSeqMax, s0->rg_k, s0->rg_v, s0);
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
    L2Z_TRY(wide_end(call, *pass));
    L2Z_HIP(hipStreamSynchronize(st));
    memcpy(out_next, b->h_next, (size_t)n * 4);
    return L2Z_OK;
}
