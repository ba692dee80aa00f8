// mixed_plan.h -- the layout of one l2z_step_mixed call (include/llama2_hip_test.h; host side: wide_host.cpp, kernels:
// mixed_step.hip) as plain C++: no HIP, nothing of the library, so tests/mixed_plan_check.cpp can build it alone under the
// sanitizers.  A call names n sequences; sequence j brings n_tokens[j] consecutive rows from position pos0[j] on, the rows
// of all sequences standing behind one another in the chunk.  A sequence of ONE row is a decode step (class "decode": the
// position-split attention), a sequence of two or more rows a prompt chunk (class "prompt": the prompt attention).  The
// plan is a pure function of (n, n_tokens, pos0).
#pragma once
#include <algorithm>
#include <cstdint>

namespace l2z {

constexpr int kMixedSeqMax = 128;    // L2Z_WIDE_MAX
constexpr int kMixedRowsMax = 512;   // L2Z_MIXED_ROWS_MAX
// a prompt sequence of r >= 2 rows has ceil(r / 64) <= r / 64 + 1 flash tiles; there are at most kMixedSeqMax of them
constexpr int kMixedTilesMax = kMixedRowsMax / 64 + kMixedSeqMax;

struct MixedPlan {
    int n = 0, R = 0;                      // sequences, rows
    int n_dec = 0;                         // one-row sequences
    int n_prompt_rows = 0;                 // rows of all sequences of two or more rows
    int n_tiles = 0;
    int deepest_dec = -1;                  // the deepest position of a one-row sequence (-1: there is none)
    int32_t seq_row0[kMixedSeqMax];        // sequence j's first row in the chunk
    int32_t row_seq[kMixedRowsMax];        // row -> sequence
    int32_t row_pos[kMixedRowsMax];        // row -> position
    int32_t dec_row[kMixedSeqMax];         // the decode list, in sequence order: entry i = (row, sequence)
    int32_t dec_seq[kMixedSeqMax];
    int32_t prompt_rows[kMixedRowsMax];    // the rows of the prompt class, ascending
    int32_t tile_seq[kMixedTilesMax];      // the flash tiles: up to 64 consecutive rows of ONE prompt sequence from row
    int32_t tile_q0[kMixedTilesMax];       // tile_q0 of that sequence on; the tiles with the most key rows first
    int32_t last_row[kMixedSeqMax];        // sequence j's last row in the chunk
};

// false (*p untouched): n outside [1, kMixedSeqMax], an n_tokens[j] < 1, more than kMixedRowsMax rows,
// or a negative position
inline bool mixed_plan(int n, const int32_t *n_tokens, const int32_t *pos0, MixedPlan *p)
{
    if (n < 1 || n > kMixedSeqMax || n_tokens == nullptr || pos0 == nullptr || p == nullptr) return false;
    long long rows = 0;
    for (int j = 0; j < n; j++) {
        if (n_tokens[j] < 1 || pos0[j] < 0) return false;
        rows += n_tokens[j];
        if (rows > kMixedRowsMax) return false;
    }
    *p = MixedPlan();
    p->n = n;
    p->R = (int)rows;
    int keys[kMixedTilesMax];   // key rows of a tile: its last query's position + 1, less one
    for (int j = 0, r = 0; j < n; j++) {
        const int m = n_tokens[j];
        p->seq_row0[j] = r;
        p->last_row[j] = r + m - 1;
        if (m == 1) {
            p->dec_row[p->n_dec] = r;
            p->dec_seq[p->n_dec++] = j;
            p->deepest_dec = std::max(p->deepest_dec, (int)pos0[j]);
        } else {
            for (int q0 = 0; q0 < m; q0 += 64) {
                p->tile_seq[p->n_tiles] = j;
                p->tile_q0[p->n_tiles] = q0;
                keys[p->n_tiles++] = pos0[j] + std::min(q0 + 63, m - 1);
            }
        }
        for (int k = 0; k < m; k++, r++) {
            p->row_seq[r] = j;
            p->row_pos[r] = pos0[j] + k;
            if (m > 1) p->prompt_rows[p->n_prompt_rows++] = r;
        }
    }
    // blocks are dispatched in id order: the tiles with the most key rows first (scheduling only, a stable insertion sort)
    for (int i = 1; i < p->n_tiles; i++) {
        const int k = keys[i], s = p->tile_seq[i], q = p->tile_q0[i];
        int at = i;
        for (; at > 0 && keys[at - 1] < k; at--) {
            keys[at] = keys[at - 1];
            p->tile_seq[at] = p->tile_seq[at - 1];
            p->tile_q0[at] = p->tile_q0[at - 1];
        }
        keys[at] = k; p->tile_seq[at] = s; p->tile_q0[at] = q;
    }
    return true;
}

}  // namespace l2z
