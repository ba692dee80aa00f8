"""The session walks of tests/q8_session_model.py run DRY, without a GPU: ref_q8's "f32" mode stands in the device's place
and is held to the "f64" mode by the same checks the device gets.  What is tested here is the walk itself -- its schedule is
a function of the seed, it reaches every operation, refusal and edge that q8_session_model.coverage lists -- and that the
reference alone stays well inside the bars the live walks are held to: at most 2 % of the compared rows are exceptions (live:
5 %), at most 5 % of the id comparisons fall under the margin.

HOW THE SEEDS WERE PICKED: seeds 1 .. 24 were run dry on each world.  A seed qualified if its coverage list was empty, and
the two seeds of a world with the smallest exception share under the rule in force (no healing: an exception's later rows are
compared as they are) were taken -- for g64 the first of them among the seeds that also meet the split coverage at SPLIT_POS.  The shares of the sweep:
profiles/q8_session_walk.md."""
import numpy as np
import pytest

import q8_session_model as qm

SEEDS = {"kv24": (10, 5), "g64": (8, 7), "kv24-flat": (5, 17)}
SPLIT_POS = 8   # L2Z_ATTN_SPLIT_POS of the graph-variant walk
SPLIT_WALK = ("g64", 8)    # a committed g64 walk whose stepped and looped calls lie on both sides of SPLIT_POS
HEAL_WALK = ("kv24", 2)    # 13.9 % of its rows are exceptions under the plain rule: one early flip, counted in every later row
WALKS = [(world, seed) for world in qm.SHAPES for seed in SEEDS[world]]
DRY_EXCEPTIONS, LIVE_EXCEPTIONS, UNDER_MARGIN = 0.02, 0.05, 0.05

_worlds, _stats = {}, {}


def dry_world(pkg, name):
    if name not in _worlds:
        _worlds[name] = qm.World(pkg, name)
    return _worlds[name]


def dry_walk(pkg, name, seed):
    """the statistics of the dry walk, each walked once a process (the GPU file compares its counts with them)"""
    if (name, seed) not in _stats:
        _stats[name, seed] = qm.run(dry_world(pkg, name), seed)
    return _stats[name, seed]


@pytest.mark.parametrize("world,seed", WALKS)
def test_the_dry_walk_holds_and_covers_everything(pkg, world, seed):
    st = dry_walk(pkg, world, seed)
    print(f"dry walk {world} seed {seed}: {st['calls']} operations, {st['exceptions']} exceptions of {st['rows']} rows "
          f"({100 * st['exc_share']:.2f} %), worst {st['worst']:.3e} of the scale, {st['id_under']} of {st['id_total']} ids under "
          f"the margin, operations {dict(st['ops'])}, refusals {dict(st['refusals'])}")
    assert len(st["log"]) == 120 + 1
    assert qm.coverage(st) == []
    assert st["exc_share"] <= DRY_EXCEPTIONS, (st["exceptions"], st["rows"])
    assert st["id_total"] >= 100 and st["under_share"] <= UNDER_MARGIN, (st["id_under"], st["id_total"])
    # the ids of mid-loop, whose rows nobody can read: another id than the reference's under the loose margin can only come
    # from an exception row, so its share is capped as the exceptions' is
    assert st["blind_total"] >= 25 and st["soft_share"] <= DRY_EXCEPTIONS, (st["blind_soft"], st["blind_total"])
    assert st["rows"] >= 1000 and st["end_rows"] >= 2 * qm.N_SEQ


def test_the_split_walk_lies_on_both_sides_of_the_switch(pkg):
    assert qm.split_coverage(dry_walk(pkg, *SPLIT_WALK), SPLIT_POS) == []


def test_the_fallback_rule_heals_a_walk_the_plain_rule_fails(pkg):
    """Walk(heal=True): the reference takes the device's K / V rows of an excepted position, so one flip is one exception"""
    plain = qm.run(dry_world(pkg, HEAL_WALK[0]), HEAL_WALK[1])
    healed = qm.run(dry_world(pkg, HEAL_WALK[0]), HEAL_WALK[1], heal=True)
    print(f"{HEAL_WALK}: plain {plain['exceptions']} of {plain['rows']}, healed {healed['exceptions']} of {healed['rows']}")
    assert plain["exc_share"] > DRY_EXCEPTIONS >= healed["exc_share"] > 0
    assert healed["end_exceptions"] < plain["end_exceptions"]   # the healed positions' rows are the device's own
    assert qm.counts(healed) == qm.counts(plain) and qm.schedule(healed) == qm.schedule(plain)


def test_the_schedule_is_a_function_of_the_seed(pkg):
    world, seed = WALKS[0]
    again = qm.run(qm.World(pkg, world), seed)
    first = dry_walk(pkg, world, seed)
    assert again["log"] == first["log"] and qm.counts(again) == qm.counts(first)
    assert qm.schedule(first) != qm.schedule(dry_walk(pkg, world, SEEDS[world][1]))


def test_stop_at_replays_a_prefix(pkg):
    world, seed = WALKS[0]
    whole = dry_walk(pkg, world, seed)["log"]
    part = qm.run(qm.World(pkg, world), seed, stop_at=30)["log"]
    assert part[-1]["op"] == "end" and 31 <= len(part) - 1 <= 32
    assert part[:-1] == whole[: len(part) - 1]


def test_the_dry_device_is_not_the_reference(pkg):
    """the walk compares two arithmetics: over the committed walks some row left the parity bar"""
    assert sum(dry_walk(pkg, w, s)["exceptions"] for w, s in WALKS) > 0


def test_the_flat_premises(pkg):
    """kv24-flat: the quantized wq is all zero in both objects, so every score is exactly 0 and every softmax weight of the
    float64 reference is exactly 1 / (pos + 1)"""
    import ref_q8
    W = dry_world(pkg, "kv24-flat")
    for k in "ab":
        q, s = W.t[k]["wq"]
        assert not q.any() and not s.any()
    m = ref_q8.Q8Model(W.cfg, W.t["a"], W.gs["a"], "f64")
    seen = []
    exp = np.exp

    class Probe:   # numpy's exp as the reference calls it in its softmax: dtype given, the scores' row as argument
        @staticmethod
        def exp(x, *a, **kw):
            out = exp(x, *a, **kw)
            if kw.get("dtype") is np.float64 and np.ndim(x) == 1 and np.size(x) <= W.cfg.seq_len and not np.any(x):
                seen.append(out / out.sum())
            return out

        def __getattr__(self, name):
            return getattr(np, name)
    ref_q8.np = Probe()
    try:
        toks = np.random.default_rng(3).integers(2, W.cfg.vocab_size, 70)
        for p, t in enumerate(toks):
            m.transformer(int(t), p)
    finally:
        ref_q8.np = np
    heads = W.cfg.n_layers * W.cfg.n_heads
    assert len(seen) >= heads * len(toks)   # every softmax of every head had all-zero scores
    assert all(np.all(w == 1.0 / w.size) for w in seen)
    # ... and a row that lands one slot off moves the output by a whole share: the V rows differ from position to position
    assert np.abs(m.vc[0, 1] - m.vc[0, 2]).max() > 1e-3


def test_the_model_s_rules():
    assert qm.accept([5, 6, 7, 8], [6, 7, 9, 1]) == 2 and qm.first_max(np.array([1.0, 3.0, 3.0], np.float32)) == 1
    e = qm.WalkFailure(7, 1, [(1, "x")], [dict(i=0, op="prefill_q8"), dict(i=1, op="trim")])
    assert e.seed == 7 and "seed=7" in str(e) and "'op': 'trim'" in str(e)
