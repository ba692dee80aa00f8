"""What l2z_verify_batch exists for: on the 7B shape, the speculative rows of four sequences (4 x 4) verified in one call take
less time than four l2z_verify calls.  A pass of up to 16 rows is bound by streaming the 26 GB of weights once; the loop
streams them four times.  DESIGN.md 4.11's step times predict a ratio near 2.9, so the condition is only "faster than the
loop"; the ratio is written down in profiles/verify_batch_bench.md (scripts/verify_batch_bench.py), not asserted."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_4_by_4_rows_in_one_call_beat_the_loop_of_verify_calls(gpu, ck):
    cfg = ck.LLAMA2_7B
    w = gpu.Weights(cfg, None, False, seed=2024)
    states = [gpu.RunState(cfg) for _ in range(4)]
    rng = np.random.default_rng(5)
    for s in states:   # histories: 16-token prefills
        s.prefill(np.array([1] + rng.integers(2, cfg.vocab_size, 15).tolist(), np.int32), 0, w)
    lists = [rng.integers(2, cfg.vocab_size, 4).astype(np.int32) for _ in states]

    def loop():
        for s, t in zip(states, lists):
            s.verify(t, 16, w)

    def batch():
        gpu.verify_batch(states, lists, 16, w)

    loop(); batch()   # warm-up: allocations, code objects
    t_loop, t_batch = [], []
    for _ in range(5):   # the two forms alternately (both calls are synchronous)
        for f, out in ((loop, t_loop), (batch, t_batch)):
            t0 = time.perf_counter()
            f()
            out.append((time.perf_counter() - t0) * 1e3)
    t_loop, t_batch = min(t_loop), min(t_batch)
    print(f"4 x 4 rows at pos 16, 7B shape: loop of l2z_verify {t_loop:.2f} ms, l2z_verify_batch {t_batch:.2f} ms "
          f"({t_loop / t_batch:.2f} x)")
    assert t_batch < t_loop
    for s in states:
        s.close()
    w.close()
