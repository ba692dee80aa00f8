// prefill_batch_host.cpp -- host side of l2z_prefill_batch (include/llama2_hip_test.h): the prompts of up to L2Z_BATCH_MAX
// sequences, one runstate each, in ONE pass of the batched prompt path -- every weight matrix streamed once per chunk of
// the CONCATENATED rows instead of once per sequence.  The pass is l2z_prefill's (prefill_host.cpp) on states[0]'s
// stream and scratch; only the q | k | v epilogue and the attention know which sequence a row belongs to
// (prefill_ragged.hip), by a small table built here per chunk.
#include <algorithm>
#include <cstring>
#include <vector>

#include "batch_host.h"

using namespace l2z;

namespace {

// the table of a chunk of P rows as one device allocation: [kRaggedMaxSeq] RaggedSeq | row_seq [cap] | row_pos [cap] | tiles
size_t tab_tiles_max(int cap) { return (size_t)cap / 64 + kRaggedMaxSeq; }
size_t tab_bytes(int cap) { return kRaggedMaxSeq * sizeof(RaggedSeq) + (size_t)cap * 8 + tab_tiles_max(cap) * sizeof(int2); }

}  // namespace

// (l2z_step_mixed takes rg_k / rg_v from here too: wide_host.cpp)
int l2z::ragged_alloc(l2z_runstate *s, int need)
{
    if (s->rg_cap >= need) return L2Z_OK;
    const size_t P = (size_t)(need + 511) / 512 * 512;   // as prefill_alloc
    const size_t kvd = (size_t)s->sh.kvd_loc;
    L2Z_HIP(hipStreamSynchronize(s->stream));
    void **bufs[] = {(void **)&s->rg_k, (void **)&s->rg_v, &s->rg_tab};
    for (void **b : bufs)
        if (*b) { (void)hipFree(*b); *b = nullptr; }
    s->rg_cap = 0;
    // (after a failure, what was allocated is freed with the runstate)
    L2Z_TRY(alloc_all("l2z_prefill_batch scratch",
                      {{(void **)&s->rg_k, P * kvd * 4}, {(void **)&s->rg_v, P * kvd * 4}, {&s->rg_tab, tab_bytes((int)P)}}));
    s->rg_cap = (int)P;
    return L2Z_OK;
}

extern "C" int l2z_prefill_batch(int n, const int32_t *tokens, const int32_t *n_tokens, const int32_t *pos0,
                                 const l2z_config *config, l2z_runstate *const *states, const l2z_weights *w)
{
    // ---- checks: a refusal enqueues nothing and changes no state ----
    L2Z_TRY(no_device_check());
    L2Z_CHECK(n_tokens != nullptr, L2Z_ERR_INVALID, "l2z_prefill_batch: null argument");
    const RaggedCall call = {"l2z_prefill_batch", n, tokens, n_tokens, pos0, 1, nullptr, nullptr, nullptr, false,
                             config, states, w, kRaggedMaxSeq, 0, 0};
    RaggedTotals t;
    L2Z_TRY(check_ragged_call(call, &t));
    const int total = t.R;
    l2z_runstate *s0 = states[0];
    hipStream_t st = s0->stream;
    const l2z_config &c = *config;
    L2Z_HIP(hipSetDevice(s0->device));
    int longest = 0;   // the plan's longest chunk sizes the scratch before anything is enqueued
    for (int done = 0; done < total;) {
        const int P = prefill_next_chunk_of(c, total - done);
        longest = std::max(longest, P);
        done += P;
    }
    L2Z_TRY(prefill_scratch(s0, longest));
    L2Z_TRY(ragged_alloc(s0, longest));

    // ---- the pass, on states[0]'s stream: it waits for every runstate's stream ... ----
    L2Z_TRY(batch_alloc(s0));  // (the events)
    L2Z_TRY(kv_attach("l2z_prefill_batch", n, states, pos0, n_tokens, 0));   // (paged runstates: the last refusal)
    L2Z_TRY(join_streams(s0->bt, n, states));
    L2Z_TRY(kv_upload(n, states, st));
    int first[kRaggedMaxSeq];   // a sequence's first row among the concatenated rows
    for (int j = 0, g = 0; j < n; g += n_tokens[j], j++) first[j] = g;
    std::vector<unsigned char> h_tab(tab_bytes(s0->rg_cap));
    struct Tile { int slot, q0, keys; };
    std::vector<Tile> tiles;
    for (int done = 0; done < total;) {
        const int P = prefill_next_chunk_of(c, total - done);
        // the chunk's table: the sequences with rows in [done, done + P), in order
        RaggedSeq *h_seq = (RaggedSeq *)h_tab.data();
        int *h_row_seq = (int *)(h_seq + kRaggedMaxSeq), *h_row_pos = h_row_seq + s0->rg_cap;
        int2 *h_tiles = (int2 *)(h_row_pos + s0->rg_cap);
        memset(h_seq, 0, kRaggedMaxSeq * sizeof(RaggedSeq));
        int n_seq = 0;
        int ends[kRaggedMaxSeq], n_ends = 0;   // sequences whose last row is in this chunk, and that row
        int end_row[kRaggedMaxSeq];
        tiles.clear();
        for (int j = 0; j < n; j++) {
            const int lo = std::max(first[j], done), hi = std::min(first[j] + n_tokens[j], done + P);
            if (lo >= hi) continue;
            RaggedSeq &q = h_seq[n_seq];
            kv_seq_base(states[j], &q);
            q.row0 = lo - done; q.rows = hi - lo; q.pos0 = pos0[j] + (lo - first[j]);
            for (int r = 0; r < q.rows; r++) { h_row_seq[q.row0 + r] = n_seq; h_row_pos[q.row0 + r] = q.pos0 + r; }
            for (int q0 = 0; q0 < q.rows; q0 += 64) tiles.push_back({n_seq, q0, q.pos0 + std::min(q0 + 63, q.rows - 1)});
            if (hi == first[j] + n_tokens[j]) { ends[n_ends] = j; end_row[n_ends++] = hi - 1 - done; }
            n_seq++;
        }
        // blocks are dispatched in id order: the tiles with the most key rows first (scheduling only: no bit depends on it)
        std::stable_sort(tiles.begin(), tiles.end(), [](const Tile &a, const Tile &b) { return a.keys > b.keys; });
        L2Z_CHECK(tiles.size() <= tab_tiles_max(s0->rg_cap), L2Z_ERR_INVALID, "l2z_prefill_batch: tile table overflow");
        for (size_t i = 0; i < tiles.size(); i++) h_tiles[i] = make_int2(tiles[i].slot, tiles[i].q0);
        unsigned char *d_tab = (unsigned char *)s0->rg_tab;
        RaggedChunk rg = {};
        rg.seq = (const RaggedSeq *)d_tab;
        rg.row_seq = (const int *)(d_tab + ((unsigned char *)h_row_seq - h_tab.data()));
        rg.row_pos = (const int *)(d_tab + ((unsigned char *)h_row_pos - h_tab.data()));
        rg.tiles = (const int2 *)(d_tab + ((unsigned char *)h_tiles - h_tab.data()));
        rg.n_seq = n_seq; rg.n_tiles = (int)tiles.size();
        rg.seq_max = kRaggedMaxSeq;
        rg.k = s0->rg_k; rg.v = s0->rg_v;
        rg.page_floats = kv_page_floats(s0);
        L2Z_HIP(hipMemcpyAsync(d_tab, h_tab.data(), h_tab.size(), hipMemcpyHostToDevice, st));
        L2Z_TRY(prefill_ragged_chunk(s0, w, tokens + done, P, rg));
        // the last residual row of every sequence that ends here is that runstate's x
        for (int e = 0; e < n_ends; e++)
            L2Z_HIP(hipMemcpyAsync(states[ends[e]]->x, s0->pf_x + (size_t)end_row[e] * c.dim, (size_t)c.dim * 4,
                                   hipMemcpyDeviceToDevice, st));
        L2Z_HIP(hipStreamSynchronize(st));  // the host table and the caller's tokens may now be reused
        done += P;
    }
    // ---- ... and every runstate's stream waits for the pass: the usual final rmsnorm + classifier launch (:426-429) of
    // each runstate, on its own stream, leaves its logits in place ----
    L2Z_TRY(release_streams(s0->bt, n, states));
    int last_pos[kRaggedMaxSeq], last_tok[kRaggedMaxSeq];
    for (int j = 0; j < n; j++) {
        l2z_runstate *s = states[j];
        last_pos[j] = pos0[j] + n_tokens[j] - 1;
        last_tok[j] = tokens[first[j] + n_tokens[j] - 1];
        L2Z_HIP(hipMemcpyAsync(s->d_pos, &last_pos[j], sizeof(int), hipMemcpyHostToDevice, s->stream));
        L2Z_HIP(hipMemcpyAsync(s->d_token, &last_tok[j], sizeof(int), hipMemcpyHostToDevice, s->stream));
        L2Z_TRY(prefill_last_logits(s, w));
    }
    for (int j = 0; j < n; j++) {
        l2z_runstate *s = states[j];
        L2Z_HIP(hipStreamSynchronize(s->stream));
        s->logits_partial = false;
        s->host_pos = pos0[j] + n_tokens[j];
    }
    return L2Z_OK;
}
