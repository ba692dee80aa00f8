// mixed_plan_check.cpp -- a stand-alone program over llama2.zig_amd/csrc/mixed_plan.h alone (no HIP, nothing of the
// library): the layout of an l2z_step_mixed call, case by case.  tests/test_mixed_plan_host.py builds it with
// -fsanitize=address,undefined and runs it; it prints one line per case and exits 0 when every check held.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "mixed_plan.h"

using namespace l2z;

static int g_failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            g_failed++;                                                  \
        }                                                                \
    } while (0)

// Everything the header promises of a plan, from (n, n_tokens, pos0) alone.  The plan lives on the heap, exactly its own
// size, so that a write past one of its arrays is the sanitizer's to report.
static void check_layout(const std::vector<int32_t> &nt, const std::vector<int32_t> &p0)
{
    const int n = (int)nt.size();
    auto pl = std::make_unique<MixedPlan>();
    CHECK(mixed_plan(n, nt.data(), p0.data(), pl.get()));
    const MixedPlan &p = *pl;
    int R = 0, n_dec = 0, n_prompt = 0, tiles = 0, deepest = -1;
    for (int j = 0; j < n; j++) {
        R += nt[j];
        if (nt[j] == 1) { n_dec++; if (p0[j] > deepest) deepest = p0[j]; }
        else { n_prompt += nt[j]; tiles += (nt[j] + 63) / 64; }
    }
    CHECK(p.n == n && p.R == R && p.n_dec == n_dec && p.n_prompt_rows == n_prompt && p.n_tiles == tiles && p.deepest_dec == deepest);
    CHECK(p.R <= kMixedRowsMax && p.n_dec <= kMixedSeqMax && p.n_tiles <= kMixedTilesMax);
    // rows -> sequences and positions: the sequences' rows behind one another
    for (int j = 0, r = 0; j < n; j++) {
        CHECK(p.seq_row0[j] == r && p.last_row[j] == r + nt[j] - 1);
        for (int k = 0; k < nt[j]; k++, r++) CHECK(p.row_seq[r] == j && p.row_pos[r] == p0[j] + k);
    }
    // every row is named exactly once: by the decode list or by the prompt rows, never both; the tiles cover the prompt
    // rows exactly once too
    std::vector<int> by_class(R, 0), by_tile(R, 0);
    for (int i = 0; i < p.n_dec; i++) {
        const int r = p.dec_row[i], j = p.dec_seq[i];
        CHECK(r >= 0 && r < R && j >= 0 && j < n);
        if (r < 0 || r >= R || j < 0 || j >= n) continue;
        CHECK(nt[j] == 1 && p.row_seq[r] == j && p.seq_row0[j] == r);
        CHECK(i == 0 || p.dec_seq[i - 1] < j);   // in sequence order: the ordinal of a decode row is a function of the layout
        by_class[r]++;
    }
    for (int i = 0; i < p.n_prompt_rows; i++) {
        const int r = p.prompt_rows[i];
        CHECK(r >= 0 && r < R);
        if (r < 0 || r >= R) continue;
        CHECK(nt[p.row_seq[r]] >= 2);
        CHECK(i == 0 || p.prompt_rows[i - 1] < r);
        by_class[r]++;
    }
    for (int r = 0; r < R; r++) CHECK(by_class[r] == 1);
    int prev_keys = 1 << 30;
    for (int i = 0; i < p.n_tiles; i++) {
        const int j = p.tile_seq[i], q0 = p.tile_q0[i];
        CHECK(j >= 0 && j < n);
        if (j < 0 || j >= n) continue;
        CHECK(nt[j] >= 2 && q0 >= 0 && q0 < nt[j] && q0 % 64 == 0);   // a tile never crosses a sequence: its rows are the sequence's own
        const int last = q0 + 63 < nt[j] - 1 ? q0 + 63 : nt[j] - 1;
        for (int q = q0; q <= last; q++) by_tile[p.seq_row0[j] + q]++;
        const int keys = p0[j] + last;
        CHECK(keys <= prev_keys);   // the tiles with the most key rows first
        prev_keys = keys;
    }
    for (int r = 0; r < R; r++) CHECK(by_tile[r] == (nt[p.row_seq[r]] >= 2 ? 1 : 0));
}

static void run(const char *name, void (*fn)())
{
    const int before = g_failed;
    fn();
    printf("%s: %s\n", g_failed == before ? "ok" : "FAILED", name);
}

int main()
{
    run("one sequence of one row", [] { check_layout({1}, {0}); check_layout({1}, {319}); });
    run("128 sequences, 512 rows", [] {
        std::vector<int32_t> nt(128, 4), p0(128);
        for (int j = 0; j < 128; j++) p0[j] = 3 * j;
        check_layout(nt, p0);
        // 127 one-row sequences and one prompt of 385 rows: seven tiles, the decode list at its longest but one
        std::vector<int32_t> nt2(128, 1), q0(128, 63);
        nt2[77] = 385; q0[77] = 60;
        check_layout(nt2, q0);
        // 128 one-row sequences: the decode list full, no tile
        check_layout(std::vector<int32_t>(128, 1), p0);
        // one prompt of 512 rows: eight tiles
        check_layout({512}, {0});
        // 128 prompts of two rows with 256 rows to spare: the most tiles a call can have when every tile is short ...
        check_layout(std::vector<int32_t>(128, 2), p0);
        // ... and 120 short prompts beside one that fills the rows: 120 + 5 tiles
        std::vector<int32_t> nt3(121, 2);
        nt3[5] = 512 - 240;
        check_layout(nt3, std::vector<int32_t>(121, 7));
    });
    run("a mix of the classes", [] {
        check_layout({1, 2, 64, 1, 65, 70, 1, 1}, {0, 5, 0, 63, 0, 60, 64, 319});
        check_layout({3, 1, 1, 130}, {10, 11, 200, 62});
    });
    run("the deepest one-row sequence sizes the decode grid", [] {
        auto pl = std::make_unique<MixedPlan>();
        const int32_t nt[] = {1, 200, 1}, p0[] = {5, 300, 130};
        CHECK(mixed_plan(3, nt, p0, pl.get()) && pl->deepest_dec == 130);   // the prompt at 300 .. 499 does not count
        const int32_t nt2[] = {2, 2}, q0[] = {5, 6};
        CHECK(mixed_plan(2, nt2, q0, pl.get()) && pl->deepest_dec == -1 && pl->n_dec == 0);
    });
    run("tiles are ordered by key rows, ties in sequence order", [] {
        auto pl = std::make_unique<MixedPlan>();
        const int32_t nt[] = {130, 2, 64, 64}, p0[] = {0, 500, 10, 10};
        CHECK(mixed_plan(4, nt, p0, pl.get()) && pl->n_tiles == 6);
        const int want_seq[] = {1, 0, 0, 2, 3, 0}, want_q0[] = {0, 128, 64, 0, 0, 0};   // keys 501, 129, 127, 73, 73, 63
        for (int i = 0; i < 6; i++) CHECK(pl->tile_seq[i] == want_seq[i] && pl->tile_q0[i] == want_q0[i]);
    });
    run("refusals", [] {
        auto pl = std::make_unique<MixedPlan>();
        const int32_t one[] = {1}, zero[] = {0}, neg[] = {-1}, big[] = {513}, two[] = {256, 257}, pos[] = {0, 0};
        CHECK(!mixed_plan(0, one, pos, pl.get()));
        CHECK(!mixed_plan(129, one, pos, pl.get()));   // (refused before anything is read)
        CHECK(!mixed_plan(1, zero, pos, pl.get()));
        CHECK(!mixed_plan(1, neg, pos, pl.get()));
        CHECK(!mixed_plan(1, big, pos, pl.get()));
        CHECK(!mixed_plan(2, two, pos, pl.get()));
        CHECK(!mixed_plan(1, one, neg, pl.get()));
        CHECK(!mixed_plan(1, nullptr, pos, pl.get()) && !mixed_plan(1, one, nullptr, pl.get()) && !mixed_plan(1, one, pos, nullptr));
        const int32_t huge[] = {2147483647, 2147483647};
        CHECK(!mixed_plan(2, huge, pos, pl.get()));   // (the row count does not wrap)
    });
    if (g_failed) printf("%d checks FAILED\n", g_failed);
    return g_failed ? 1 : 0;
}
