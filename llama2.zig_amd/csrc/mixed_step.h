// mixed_step.h -- what l2z_step_mixed adds to the ragged prompt pass (mixed_step.hip; host side wide_host.cpp; the layout:
// mixed_plan.h): the device table of a chunk that holds sequences of ONE row (decode steps) and sequences of several rows
// (prompt chunks), the attention dispatch for such a chunk -- which wide_host.cpp hands to the pass as the chunk's
// attention (RaggedChunk::attention); the layer loop itself does not know this file -- and the last launch of the call:
// every sequence's draw from its LAST row's logits and the hand-out of that row to the runstate.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "l2z_internal.h"
#include "mixed_plan.h"

namespace l2z {

// What the host uploads before the pass, in one copy from a pinned buffer.  seq / row_seq / pos are the table
// launch_ragged_rope_scatter and the prompt attention read (RaggedChunk); cache bases are layer 0's.
struct MixedTable {
    RaggedSeq seq[kMixedSeqMax];           // slot j = sequence j: caches, row0, rows, pos0
    int32_t row_seq[kMixedRowsMax];
    int32_t pos[kMixedRowsMax];
    int32_t tokens[kMixedRowsMax];
    float *logits[kMixedSeqMax];           // sequence j's runstate's logits
    int2 dec[kMixedSeqMax];                // the decode list: .x the row, .y the sequence slot
    int32_t last_row[kMixedSeqMax];
    int32_t prompt_rows[kMixedRowsMax];    // the rows of the sequences of several rows
    int2 tiles[kMixedTilesMax];            // RaggedChunk::tiles, those sequences' only
    float temperature[kMixedSeqMax], top_p[kMixedSeqMax], coins[kMixedSeqMax];   // per SEQUENCE
};

struct MixedAttn {
    const MixedTable *tab;   // device
    float *part;             // wide_part_floats (wide_decode.h): indexed by a decode row's ORDINAL in the list, < kMixedSeqMax
    int seg_cap;             // verify_segments(seq_len)
    int n_seg;               // segments of the deepest one-row sequence: the decode grid's extent
    int n_dec;               // entries of tab->dec
    int n_prompt_rows;       // entries of tab->prompt_rows
    size_t page_floats;      // RaggedChunk::page_floats
};

// The attention of a mixed chunk, rows of q [P, ldq] (RoPE applied) into out [P, ldo]: the layer as the ragged pass
// describes it (RaggedLayer), this call's MixedAttn, and the chunk's table as the pass holds it.
//   the sequences of several rows: launch_ragged_attention (prefill_ragged.hip) over rg.tiles (head sizes 64 / 128) or over
//     the rows rg.att_rows names (every other head size);
//   the sequences of one row: launch_wide_attention_rows (wide_decode.h) with tab->dec as the list -- block (kv head x part,
//     segment, ordinal) takes its row and its sequence slot from tab->dec[ordinal], reads the segment's K / V rows of that kv
//     head ONCE for its query heads (one page per block when paged) and leaves the partials at the ORDINAL; the combine,
//     block (head, ordinal), folds them in segment order into the row.
// No block is launched for a row of the other class.  L.x3 / L.kp / planes_written as launch_ragged_attention: the planes of
// bf16 terms of out are written by BOTH classes' launches (the flash form and the combine) or by neither.
hipError_t launch_mixed_attention(const RaggedLayer &L, const MixedAttn &m, const RaggedChunk &rg, bool *planes_written = nullptr);

// The last launch, one block of 1024 threads per SEQUENCE: next[j] = the token the sampler's row body (sample_device.h)
// draws from row j of logits [n, ld] with tab->temperature[j], top_p[j], coins[j] -- the argmax by argmax_rule.h at
// temperature 0 or !sampled, where neither coin nor scratch is read -- and row j -> tab->logits[j].
struct MixedDraw {
    const float *logits;
    int ld, vocab;
    const MixedTable *tab;
    bool sampled;
    float *scratch;        // row_stride floats per sequence, sample_scratch_floats(vocab) at least; null: all greedy
    size_t row_stride;
    int *next;             // [n]
};
hipError_t launch_mixed_draw_out(const MixedDraw &d, int n, hipStream_t st);

}  // namespace l2z
