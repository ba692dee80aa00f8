// wide_decode.h -- the kernels l2z_transformer_wide adds to the ragged prompt pass (wide_decode.hip; host side
// wide_host.cpp, prefill_host.cpp): decode attention for up to kWideMax one-query sequences, each on its own cache (the
// verify family's segment body, verify_device.h, with a kv head's query heads as a block's slots), and the launch that
// hands the [n, vocab] logits matrix back to the runstates.  Every row's token, position, caches and
// logits come from one device table.  And the last launch of a step inside l2z_wide_run (wide_sample.hip): every row's
// draw, and the hand-over of token and position to the next step on the device.  And what l2z_verify_wide puts in their
// place (wide_verify.hip): attention whose slots are the rows of ONE sequence, and the verdict per sequence.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "batch_decode.h"
#include "l2z_internal.h"

namespace l2z {

constexpr int kWideMax = 128;  // L2Z_WIDE_MAX

// What the host uploads before a step, in one copy from a pinned buffer.  The first three arrays are the table
// launch_ragged_rope_scatter reads (RaggedChunk: kWideMax sequence slots of one row each, row i = slot i); cache bases are
// layer 0's.
struct WideTable {
    RaggedSeq seq[kWideMax];      // kc, vc of row i's runstate; row0 = i, rows = 1, pos0 = pos[i]
    int32_t row_seq[kWideMax];    // i
    int32_t pos[kWideMax];
    int32_t tokens[kWideMax];
    float *logits[kWideMax];
};

// Segments of kVerifySeg ABSOLUTE positions, the verify family's scheme: segment s = positions [s * kVerifySeg,
// (s + 1) * kVerifySeg) whatever n and the positions are.
// Partials of one step: [kWideMax, n_heads, seg_cap, head_size] sums, then [kWideMax, n_heads, seg_cap, 2] (max, sum e),
// in one allocation of kWideMax * n_heads * seg_cap * (head_size + 2) floats.
inline size_t wide_part_floats(int n_heads, int seg_cap, int head_size)
{
    return (size_t)kWideMax * n_heads * seg_cap * ((size_t)head_size + 2);
}
struct WideAttn {
    const WideTable *tab;  // device
    float *part;           // wide_part_floats
    int seg_cap;           // verify_segments(seq_len)
    int n_seg;             // segments of the deepest row of this step: the grid's extent
    int verify_m;          // 0: one row per sequence (launch_wide_attention); l2z_verify_wide: the slots of a block, the
                           // smallest of 1, 2, 4, 8, 16 that holds the call's longest sequence (launch_wide_verify_attention)
    int n_seq;             // l2z_verify_wide: the table's sequences
    size_t page_floats;    // RaggedChunk::page_floats of the step (0: contiguous caches)
};

// Every attention launcher here takes the layer's q, out, shape, cache offsets, stream and planes as the ragged pass's
// RaggedLayer (l2z_internal.h), then its own table, then planes_written.
// Decode attention (main.zig:361-389) of rows 0 .. n - 1 of q [n, ldq] (RoPE applied) into out [n, ldo], n = L.P, two launches:
//   wide_attention: block (kv head, segment, row) reads the segment's K and V rows of that kv head ONCE and serves all
//     kv_mul query heads of it (up to 4 per block; beyond, blocks of 4, the last one with the heads that are left); a block
//     past its row's last segment returns.  It leaves the flash partials (max, sum e, sum e v) per (row, head, segment).
//   wide_combine: block (head, row) folds the row's segments in segment order, divides, and writes out -- and, x3 != null,
//     out's planes of bf16 terms x3[row][3][kp] (the Wo product's operand; *planes_written says whether it did).
// head_size: a multiple of 4 up to 256.  Every summation order is verify_device.h's: a function of head_size, the segment
// and the row's own position only; no block touches two sequences.  Keys beyond pos[i] are never read.
hipError_t launch_wide_attention(const RaggedLayer &L, const WideAttn &wa, bool *planes_written = nullptr);
// The same two launches over rows named one by one (l2z_step_mixed, mixed_step.hip: the one-row sequences of a chunk that
// holds prompt rows too): block ordinal i of either launch serves row list[i].x of the chunk -- q, out, the planes, pos[] --
// on sequence slot list[i].y of seq[]; the partials stand at the ORDINAL, n <= kWideMax of them.  list == null: row = slot =
// ordinal, which is launch_wide_attention -- one kernel body for both, so the bits of a row do not depend on how it is named.
struct WideRows {
    const int32_t *pos;      // device: [rows of the chunk]
    const RaggedSeq *seq;    // device: [sequence slots]
    const int2 *list;        // device: [n], or null
    int n;
    float *part;             // wide_part_floats
    int seg_cap, n_seg;      // as WideAttn's; n_seg: segments of the deepest listed row
    size_t page_floats;
};
hipError_t launch_wide_attention_rows(const RaggedLayer &L, const WideRows &wr, bool *planes_written = nullptr);   // (wr.n rows, not L.P)
// wide_combine alone, over the partials some attention launch left for rows 0 .. n - 1 (tab->pos[row] = the row's position)
hipError_t launch_wide_combine(float *out, int ldo, const WideAttn &wa, int n, int n_heads, int head_size, hipStream_t st,
                               void *x3 = nullptr, int kp = 0, bool *planes_written = nullptr);

// Row i of logits [n, ld] -> tab->logits[i][0 .. vocab) (float4 where both sides are 16-byte aligned), and, next != null,
// next[i] = the row's argmax by argmax_rule.h (strict '>', lowest index wins).  One launch, one block per row.
hipError_t launch_wide_logits_out(const float *logits, int ld, const WideTable *tab, int vocab, int *next, int n,
                                  hipStream_t st);

// The last launch of one step of l2z_wide_run (wide_sample.hip), one block of 1024 threads per row: row i's token is drawn
// from row i of logits [n, ld] by the sampler's row body (sample_device.h: the token l2z_sample_batch draws from the same
// logits with temperature[i], top_p[i], coins[i]; the argmax by argmax_rule.h at temperature 0, the coin not read), stored
// in ids[i], and the row is handed to the next step on the device: the token into tokens[i] (the embed launch's array),
// tab->pos[i] and tab->seq[i].pos0 moved on by one.  logits_out (the run's last step): the row goes to tab->logits[i] as
// launch_wide_logits_out copies it.
struct WideDraw {
    const float *logits;
    int ld, vocab;
    WideTable *tab;
    const float *temperature, *top_p;  // [n]; temperature null: every row takes the argmax
    const float *coins;                // [n], this step's; read where temperature[i] > 0
    float *scratch;                    // row_stride floats per row, sample_scratch_floats(vocab) at least; null: all greedy
    size_t row_stride;
    int *ids;                          // [n], this step's
    int *tokens;                       // [n]
    bool logits_out;
};
hipError_t launch_wide_draw_advance(const WideDraw &d, int n, hipStream_t st);

// ---- l2z_verify_wide (wide_verify.hip): the table's sequence slot j is ONE sequence's seq[j].rows <= kBatchMax consecutive
// positions from seq[j].pos0 on, rows seq[j].row0 .. of the chunk; row_seq[r], pos[r] and tokens[r] are per row, logits[j]
// is per SEQUENCE: the runstate's logits the verdict fills ----

// Causal attention of rows 0 .. n_rows - 1 of q [n_rows, ldq] (RoPE applied) into out [n_rows, ldo], n_rows = L.P rows of
// wa.n_seq sequences, two launches:
//   wide_verify_attention<M>: block (head, segment, sequence), M = wa.verify_m; its slots are the sequence's rows of that
//     head as verify_attention_body sets them up (row i sees the keys t <= pos0 + i; the rows that end before the segment
//     are out of use), the q slices and partials addressed through the wide step's row-indexed layout.  A block past its
//     own sequence's last segment returns.  A kv head's K / V rows are read once per QUERY head here: sharing them between
//     the query heads of a kv head, as wide_attention does, needs slot strides in two dimensions.
//   wide_combine, as it stands: a row's segments 0 .. pos[row] / kVerifySeg, and the bf16 planes.
// Every summation order is verify_device.h's; no block touches two sequences.  wa.n_seg: the segments of the deepest
// sequence's last position.
hipError_t launch_wide_verify_attention(const RaggedLayer &L, const WideAttn &wa, bool *planes_written = nullptr);

// The per-sequence controls of a sampled call, behind the WideTable in the same allocations and the same copy
struct WideVerdictCtl {
    float temperature[kWideMax], top_p[kWideMax];  // per sequence
    float coins[kWideMax];                         // per row
};
// The verdict of l2z_verify_wide, two launches.  The draw: one block of 1024 threads per row, next[r] = the token the
// sampler's row body (sample_device.h) draws from row r of logits [n_rows, ld] with its sequence's temperature and top_p and
// coins[r] -- the argmax at temperature 0 or ctl == null, where neither coin nor scratch is read.  The accept: one block per
// sequence, a = the number of leading guesses tokens[row0 + i + 1] == next[row0 + i] (verify_batch_accept_kernel's scan over
// the sequence's own rows) -> accepted[j], and row row0 + a of the matrix -> tab->logits[j] (wide_logits_out's copy).
struct WideVerdict {
    const float *logits;
    int ld, vocab;
    const WideTable *tab;
    const WideVerdictCtl *ctl;  // null: every sequence greedy
    float *scratch;             // row_stride floats per row, sample_scratch_floats(vocab) at least; null: no sequence draws
    size_t row_stride;
    int *next;                  // [n_rows]
    int *accepted;              // [n_seq]
};
hipError_t launch_wide_verdict(const WideVerdict &d, int n_seq, int n_rows, hipStream_t st);

}  // namespace l2z
