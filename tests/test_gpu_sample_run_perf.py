"""l2z_sample_run against the route it replaces, measured side by side in one process: 128 generated tokens on the
stories110M shape at t = 0.05, p = 0.9, best of 3 each.  The loop removes one sync, one upload and one copy back per token and
leaves the device time as it is, so its tokens/s must be at least that of l2z_transformer + l2z_sample_batch per token.
(Measured ratios: profiles/sample_run_bench.md.)"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_the_loop_is_no_slower_than_transformer_plus_sample_batch(gpu, ck):
    cfg = ck.Config(768, 2048, 12, 12, 12, 32000, 320)
    w = gpu.Weights(cfg, None, True, seed=77)
    s = gpu.RunState(cfg)
    n, t, p = 128, 0.05, 0.9
    coins = gpu.coin_stream(1, n)

    def loop():
        s.greedy_begin(())
        t0 = time.perf_counter()
        ids = s.sample_run(w, n, t, p, coins)
        return time.perf_counter() - t0, ids

    def stepped():
        token, ids = 1, []
        t0 = time.perf_counter()
        for pos in range(n):
            s.transformer(token, pos, w)
            token = int(gpu.sample_batch([s], t, p, coins[pos])[0])
            ids.append(token)
            if token == 1:
                break
        return time.perf_counter() - t0, np.array(ids, np.int32)

    loop(); stepped()   # graphs captured, scratch allocated
    best = {}
    for name, fn in (("loop", loop), ("stepped", stepped)):
        runs = [fn() for _ in range(3)]
        best[name] = min(r[0] for r in runs)
        ids = runs[0][1]
        assert all(np.array_equal(ids, r[1]) for r in runs)
        best[name + "_ids"] = ids
    assert np.array_equal(best["loop_ids"], best["stepped_ids"])
    assert len(best["loop_ids"]) == n, "a drawn BOS ended the run: take another coin seed"
    loop_tps, stepped_tps = n / best["loop"], n / best["stepped"]
    print(f"sample_run: loop {loop_tps:.0f} tok/s, transformer + sample_batch {stepped_tps:.0f} tok/s, "
          f"ratio {loop_tps / stepped_tps:.3f}")
    assert loop_tps >= stepped_tps
    s.close(); w.close()
