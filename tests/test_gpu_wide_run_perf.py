"""What l2z_wide_run exists for: on the 7B shape, 8 sampled steps of 64 sequences in ONE call take no more time than the
loop they replace -- per step one l2z_transformer_wide call and four l2z_sample_batch calls, each of the four a launch, a
copy back and a sync, with the 63-stream join around every one of the five.  The run issues the same step launches and
draws with the same row body; it removes the four sampler launches' round trips and the per-step joins and adds nothing,
so the condition is parity (ratio loop / run >= 1.0) and the margin is whatever the measurement shows: it is written down
in DESIGN.md 4.18 and profiles/wide_run_bench.md (scripts/wide_run_bench.py), not asserted."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_8_sampled_steps_of_64_sequences_in_one_run_are_not_slower_than_the_step_loop(gpu, ck):
    c = ck.LLAMA2_7B
    cfg = ck.Config(c.dim, c.hidden_dim, c.n_layers, c.n_heads, c.n_kv_heads, c.vocab_size, 256)   # 64 caches of 256 rows
    w = gpu.Weights(cfg, None, False, seed=2024)
    n, steps = 64, 8
    states = [gpu.RunState(cfg) for _ in range(n)]
    rng = np.random.default_rng(6)
    pos = rng.integers(0, 32 - steps, n).astype(np.int32)   # every position of the run below 32
    tok = rng.integers(2, cfg.vocab_size, n).astype(np.int32)
    temp, topp = np.full(n, 1.0, np.float32), np.full(n, 0.9, np.float32)
    coins = rng.random((steps, n), np.float32)

    def loop():   # built only from entry points that stood before the run
        t = tok
        for k in range(steps):
            gpu.transformer_wide(states, t, pos + k, w, want_next=False)
            t = np.concatenate([gpu.sample_batch(states[g:g + 16], temp[g:g + 16], topp[g:g + 16], coins[k, g:g + 16])
                                for g in range(0, n, 16)])
        for s in states:
            s.synchronize()
        return t

    def run():
        ids = gpu.wide_run(states, tok, pos, w, steps, temp, topp, coins)
        for s in states:
            s.synchronize()
        return ids[-1]

    def timed(f):
        t0 = time.perf_counter()
        out = f()
        return (time.perf_counter() - t0) * 1e3, out

    a, b = loop(), run()   # warm-up: allocations, code objects -- and the same rows rewritten, so the same last ids
    assert np.array_equal(a, b)
    t_loop, t_run = [], []
    for _ in range(5):   # the two ways alternate
        t_loop.append(timed(loop)[0])
        t_run.append(timed(run)[0])
    t_loop, t_run = min(t_loop), min(t_run)
    print(f"64 sequences, 7B shape, pos < 32, 8 steps at (1.0, 0.9): the step loop {t_loop:.2f} ms ({t_loop / steps:.2f} per step), "
          f"one l2z_wide_run call {t_run:.2f} ms ({t_run / steps:.2f} per step): ratio loop / run {t_loop / t_run:.3f}")
    assert t_loop / t_run >= 1.0
    for s in states:
        s.close()
    w.close()
