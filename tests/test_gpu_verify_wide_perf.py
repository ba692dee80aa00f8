"""What l2z_verify_wide exists for: on the 7B shape, the verify pass of 16 sequences x 4 rows in one call takes no more time
than the four l2z_verify_batch calls (4 sequences x 4 rows = 16 rows each) that the same sequences need today.  A
l2z_verify_batch call is bound by streaming the 26 GB of weights once per call; the wide call streams them once for all 64
rows on the matrix cores.  The condition is only "not slower than the loop"; the measured times and the ratio are written
down in DESIGN.md 4.19 and profiles/verify_wide_bench.md (scripts/verify_wide_bench.py), not asserted."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_16_sequences_of_4_rows_in_one_wide_call_are_not_slower_than_four_verify_batch_calls(gpu, ck):
    c = ck.LLAMA2_7B
    cfg = ck.Config(c.dim, c.hidden_dim, c.n_layers, c.n_heads, c.n_kv_heads, c.vocab_size, 256)   # 16 caches of 256 rows
    w = gpu.Weights(cfg, None, False, seed=2024)
    states = [gpu.RunState(cfg) for _ in range(16)]
    rng = np.random.default_rng(5)
    pos = rng.integers(0, 28, 16).astype(np.int32)   # positions below 32 (the rows' contents do not change the work)
    lists = [rng.integers(2, cfg.vocab_size, 4).astype(np.int32) for _ in range(16)]

    def loop():
        for g in range(0, 16, 4):
            gpu.verify_batch(states[g:g + 4], lists[g:g + 4], pos[g:g + 4], w)

    def wide():
        gpu.verify_wide(states, lists, pos, w)

    for f in (loop, wide):   # warm-up: allocations, code objects
        f()
    t_loop, t_wide = [], []
    for _ in range(5):       # alternating, best of 5; both forms are synchronous calls
        for f, out in ((loop, t_loop), (wide, t_wide)):
            t0 = time.perf_counter()
            f()
            out.append((time.perf_counter() - t0) * 1e3)
    t_loop, t_wide = min(t_loop), min(t_wide)
    print(f"16 sequences x 4 rows, 7B shape, pos < 32, greedy: four l2z_verify_batch calls {t_loop:.2f} ms, one l2z_verify_wide "
          f"call {t_wide:.2f} ms (ratio {t_loop / t_wide:.2f})")
    assert t_loop / t_wide >= 1.0
    for s in states:
        s.close()
    w.close()
