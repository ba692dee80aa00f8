"""The session walks of tests/session_model.py run DRY, without a GPU: the device's outputs are replaced by the model's own
expectation (oracle logits, oracle argmax, the host sampler's draws), so what is tested here is the walk itself -- that its
schedule is a function of the seed, that it reaches every entry point, every scratch hand-over and every refusal, and that
the oracle's margins leave the id comparisons their teeth.

HOW THE SEEDS WERE PICKED: seeds 1 .. 24 were run dry on each shape (a shape's seq_len sets the length of its long prompts,
so a seed's schedule differs between shapes).  A seed qualified if, with the oracle alone, its walk met everything
session_model.coverage asks, the row totals fell on both sides of every edge, most paged calls passed, and the calls lay
on both sides of the attention switch at SPLIT_POS as session_model.split_coverage asks.  kvmul3: 6, 7, 8 qualified, hs64: 1,
2, 21.  Taken: kvmul3 6 and 8 (7 holds only four of the seven kinds of refusal), hs64 1 and 2; kvmul3 6 and both of hs64 hold
all seven kinds.  tests/test_gpu_session_walk.py runs the same walks and asserts the same coverage on the live statistics: the model's
bookkeeping, the scratch owners included, does not depend on whether a device is present."""
import numpy as np
import pytest

import session_model as sm

SEEDS = {"kvmul3": (6, 8), "hs64": (1, 2)}
SPLIT_POS = 8   # L2Z_ATTN_SPLIT_POS of the graph-variant walk: a position the stepped and the looped calls really cross
WALKS = [(shape, seed) for shape in sm.SHAPES for seed in SEEDS[shape]]

_stats = {}


@pytest.fixture(scope="module")
def walks(ck, orc):
    """(shape, seed) -> the statistics of its dry walk, each walked once"""
    worlds = {}

    def get(shape, seed):
        if (shape, seed) not in _stats:
            if shape not in worlds:
                worlds[shape] = sm.World(ck, orc, shape)
            _stats[shape, seed] = sm.run(worlds[shape], seed)
        return _stats[shape, seed]
    yield get
    _stats.clear()


@pytest.mark.parametrize("shape,seed", WALKS[:2])
def test_the_schedule_is_a_function_of_the_seed(ck, orc, walks, shape, seed):
    again = sm.run(sm.World(ck, orc, shape), seed)   # (a world of its own: no logits remembered from the first run)
    assert sm.schedule(again) == sm.schedule(walks(shape, seed))
    assert again["log"] == walks(shape, seed)["log"]
    assert sm.schedule(walks(shape, SEEDS[shape][0])) != sm.schedule(walks(shape, SEEDS[shape][1]))


@pytest.mark.parametrize("shape,seed", WALKS)
def test_every_kind_of_operation_occurs(walks, shape, seed):
    st = walks(shape, seed)
    assert len(st["log"]) == 150 + 1   # the operations and the end-of-walk entry
    assert sm.coverage(st) == []
    n_refused = sum(st["refusals"].values())
    assert 10 <= n_refused <= 30, n_refused   # about one call in ten, and what the pool refuses on top


@pytest.mark.parametrize("shape,seed", WALKS)
def test_the_scratch_owner_moves_and_the_row_totals_straddle_the_edges(walks, shape, seed):
    st = walks(shape, seed)
    assert st["owner_moved"] == set(sm.WIDE_KINDS), set(sm.WIDE_KINDS) - st["owner_moved"]
    # the many-row calls' totals on both sides of 16 | 17, 32 | 33 and 64 | 65, where the prompt pass changes its GEMM form
    rows = [e["rows"] for e in st["log"] if "rows" in e and "refusal" not in e]
    for lo, hi in ((1, 16), (17, 32), (33, 64), (65, 512)):
        assert any(lo <= r <= hi for r in rows), ((lo, hi), sorted(set(rows)))
    assert len({16, 17, 32, 33, 64, 65} & set(rows)) >= 3, sorted(set(rows))   # ... and right at the edges


@pytest.mark.parametrize("shape,seed", WALKS)
def test_calls_lie_on_both_sides_of_the_attention_switch(walks, shape, seed):
    assert sm.split_coverage(walks(shape, seed), SPLIT_POS) == []


def test_the_long_shape_reaches_its_upper_pages(walks):
    """hs64 has five page slots: its walks attach the fourth (positions from 192 on)"""
    assert all(walks("hs64", seed)["top_slot"] >= 3 for seed in SEEDS["hs64"])


@pytest.mark.parametrize("shape,seed", WALKS)
def test_the_pool_runs_dry(walks, shape, seed):
    st = walks(shape, seed)
    assert st["oom"] >= 1 and st["min_free"] == 0
    # ... while most calls on paged runstates still pass
    paged = [e for e in st["log"] if e["op"] in sm.WIDE_KINDS and e.get("seqs", ["c"])[0].startswith("p")]
    assert sum("refusal" not in e for e in paged) > len(paged) // 2


def test_every_kind_of_refusal_occurs_over_the_set(walks):
    seen = set()
    for shape, seed in WALKS:
        seen |= {k for k, n in walks(shape, seed)["refusals"].items() if n > 0}
    assert seen == set(sm.REFUSALS), set(sm.REFUSALS) - seen


@pytest.mark.parametrize("shape,seed", WALKS)
def test_few_id_comparisons_fall_under_the_margin(walks, shape, seed):
    st = walks(shape, seed)
    assert st["id_total"] >= 300
    assert st["id_under"] <= 0.05 * st["id_total"], (st["id_under"], st["id_total"])


def test_stop_at_replays_a_prefix(ck, orc, walks):
    shape, seed = WALKS[0]
    whole = walks(shape, seed)["log"]
    part = sm.run(sm.World(ck, orc, shape), seed, stop_at=40)["log"]
    assert part[-1]["op"] == "end" and 41 <= len(part) - 1 <= 42
    assert part[:-1] == whole[: len(part) - 1]


def test_a_failure_names_seed_index_and_log():
    e = sm.WalkFailure(7, 1, [(1, "x")], [dict(i=0, op="prefill"), dict(i=1, op="trim")])
    assert e.seed == 7 and e.index == 1 and "seed=7" in str(e) and "stop_at=1" in str(e) and "'op': 'trim'" in str(e)
    assert eval(repr(e.log)) == e.log   # Python literals


def test_the_models_verdict_rules():
    assert sm.accept([5, 6, 7, 8], [6, 7, 9, 1]) == 2 and sm.accept([5], [3]) == 0 and sm.accept([5, 6], [7, 6]) == 0
    #      0
    #    1   3        node 2 behind 1, node 4 behind 3
    assert sm.tree_verdict([5, 6, 7, 8, 9], [-1, 0, 1, 0, 3], [8, 0, 0, 9, 2]) == [0, 3, 4]
    assert sm.tree_verdict([5, 6], [-1, 0], [7, 6]) == [0]
    assert sm.first_max(np.array([1.0, 3.0, 3.0], np.float32)) == 1
