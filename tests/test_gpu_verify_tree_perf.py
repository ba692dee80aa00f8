"""What l2z_verify_tree exists for: on the 7B shape, one call on a 16-node tree takes less time than two l2z_verify calls of 8
rows -- what a caller with two candidate continuations makes today.  A pass of up to 16 rows is bound by streaming the 26 GB
of weights once; two chain calls stream them twice, so the condition needs no margin.  The ratios are written down in
profiles/verify_tree_bench.md (scripts/verify_tree_bench.py), not asserted."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BUSH = [-1, 0, 0, 2, 1, 3, 3, 4, 2, 5, 5, 6, 7, 8, 0, 1]   # 16 nodes, depth 4, branching at every level


def test_one_16_node_tree_call_beats_two_verify_calls_of_8_rows(gpu, ck):
    cfg = ck.LLAMA2_7B
    w = gpu.Weights(cfg, None, False, seed=2024)
    s = gpu.RunState(cfg)
    rng = np.random.default_rng(5)
    s.prefill(np.array([1] + rng.integers(2, cfg.vocab_size, 15).tolist(), np.int32), 0, w)
    toks = rng.choice(np.arange(2, cfg.vocab_size), 16, replace=False).astype(np.int32)

    def chains():
        s.verify(toks[:8], 16, w)
        s.verify(np.concatenate([toks[:1], toks[8:15]]), 16, w)

    def tree():
        s.verify_tree(toks, BUSH, 16, w)

    chains(); tree()   # warm-up: allocations, code objects
    t_chains, t_tree = [], []
    for _ in range(5):   # the two forms alternately (both calls are synchronous)
        for f, out in ((chains, t_chains), (tree, t_tree)):
            t0 = time.perf_counter()
            f()
            out.append((time.perf_counter() - t0) * 1e3)
    t_chains, t_tree = min(t_chains), min(t_tree)
    print(f"16 nodes at pos 16, 7B shape: two l2z_verify calls of 8 rows {t_chains:.2f} ms, l2z_verify_tree {t_tree:.2f} ms "
          f"({t_chains / t_tree:.2f} x)")
    assert t_tree < t_chains
    s.close()
    w.close()
