"""What l2z_prefill_batch exists for: on the 7B shape, 16 prompts of 32 tokens in one call take less time than 16 l2z_prefill
calls.  A short chunk is bound by streaming the 26 GB of weights (6.5 ms per 32-token call), one 512-row pass takes under
40 ms: more than a factor of two, so the condition is only "faster than the loop".  The ratio is written down in
profiles/prefill_batch_bench.md (scripts/prefill_batch_bench.py), not asserted."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_16_prompts_of_32_tokens_in_one_call_beat_the_loop(gpu, ck):
    cfg = ck.LLAMA2_7B
    w = gpu.Weights(cfg, None, False, seed=2024)
    states = [gpu.RunState(cfg) for _ in range(16)]
    rng = np.random.default_rng(5)
    lists = [np.array([1] + rng.integers(2, cfg.vocab_size, 31).tolist(), np.int32) for _ in states]

    def loop():
        for s, t in zip(states, lists):
            s.prefill(t, 0, w)
        for s in states:
            s.synchronize()

    def batch():
        gpu.prefill_batch(states, lists, 0, w)
        for s in states:
            s.synchronize()

    def best_of(f, rounds=5):
        f()   # warm-up: allocations, code objects
        out = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            f()
            out.append((time.perf_counter() - t0) * 1e3)
        return min(out)

    t_loop, t_batch = best_of(loop), best_of(batch)
    print(f"16 x 32 tokens, 7B shape: loop of l2z_prefill {t_loop:.2f} ms, l2z_prefill_batch {t_batch:.2f} ms "
          f"({t_loop / t_batch:.2f} x)")
    assert t_batch < t_loop
    for s in states:
        s.close()
    w.close()
