"""What l2z_step_mixed exists for: on the 7B shape, 64 decoding sequences and two newly arrived prompts of 96 rows in ONE call
take no more time than the two calls the same work needs without it -- l2z_prefill_batch for the prompts, then
l2z_transformer_wide for the decoders: two sweeps of the weights against one.  The condition is only "one sweep does not
lose to two"; the measured times and the ratio are written down in DESIGN.md 4.21 and profiles/mixed_step_bench.md
(scripts/mixed_step_bench.py)."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_one_mixed_call_is_not_slower_than_prefill_batch_then_the_wide_step(gpu, ck):
    c = ck.LLAMA2_7B
    cfg = ck.Config(c.dim, c.hidden_dim, c.n_layers, c.n_heads, c.n_kv_heads, c.vocab_size, 256)
    w = gpu.Weights(cfg, None, False, seed=2024)
    n_dec, n_pr, rows = 64, 2, 96
    rng = np.random.default_rng(7)
    pos = rng.integers(0, 32, n_dec).astype(np.int32)   # positions below 32 (the rows' contents do not change the work)
    tok = rng.integers(2, cfg.vocab_size, n_dec).astype(np.int32)
    prompts = [np.r_[1, rng.integers(2, cfg.vocab_size, rows - 1)].astype(np.int32) for _ in range(n_pr)]
    mixed_states = [gpu.RunState(cfg) for _ in range(n_dec + n_pr)]
    twins = [gpu.RunState(cfg) for _ in range(n_dec + n_pr)]
    lists = [[t] for t in tok] + prompts
    pos0 = np.r_[pos, np.zeros(n_pr, np.int32)].astype(np.int32)

    def two_calls():
        gpu.prefill_batch(twins[n_dec:], prompts, 0, w)
        gpu.transformer_wide(twins[:n_dec], tok, pos, w)

    def mixed():
        gpu.step_mixed(mixed_states, lists, pos0, w)

    for f in (two_calls, mixed):   # warm-up: allocations, code objects
        f()
    t_two, t_mixed = [], []
    for _ in range(5):             # alternating, best of 5; both forms are synchronous
        for f, out in ((two_calls, t_two), (mixed, t_mixed)):
            t0 = time.perf_counter()
            f()
            out.append((time.perf_counter() - t0) * 1e3)
    t_two, t_mixed = min(t_two), min(t_mixed)
    print(f"64 decoders at pos < 32 + 2 prompts of 96 rows, 7B shape: l2z_prefill_batch then l2z_transformer_wide {t_two:.2f} ms, "
          f"one l2z_step_mixed call {t_mixed:.2f} ms (ratio {t_two / t_mixed:.2f})")
    assert t_two / t_mixed >= 1.0
    for s in mixed_states + twins:
        s.close()
    w.close()
