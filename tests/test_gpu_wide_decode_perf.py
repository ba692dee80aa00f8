"""What l2z_transformer_wide exists for: on the 7B shape, one decode step of 64 sequences in one call takes less time than
the four l2z_transformer_batch calls of 16 that the same sequences need today.  A batched step is bound by streaming the
26 GB of weights (6.6 ms per call at short context), and the same weights multiply a 64-row chunk in about 8 ms on the
prompt pass's stream form: the condition is only "faster than the loop".  The ratio is written down in
profiles/wide_decode_bench.md (scripts/wide_bench.py), not asserted."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_64_sequences_in_one_wide_step_beat_four_batched_steps(gpu, ck):
    c = ck.LLAMA2_7B
    cfg = ck.Config(c.dim, c.hidden_dim, c.n_layers, c.n_heads, c.n_kv_heads, c.vocab_size, 256)   # 64 caches of 256 rows
    w = gpu.Weights(cfg, None, False, seed=2024)
    states = [gpu.RunState(cfg) for _ in range(64)]
    rng = np.random.default_rng(5)
    pos = rng.integers(0, 32, 64).astype(np.int32)   # (the rows' contents do not change the work: no history is fed)
    tok = rng.integers(2, cfg.vocab_size, 64).astype(np.int32)

    def loop():
        for g in range(0, 64, 16):
            gpu.transformer_batch(states[g:g + 16], tok[g:g + 16], pos[g:g + 16], w)
        for s in states:
            s.synchronize()

    def wide():
        gpu.transformer_wide(states, tok, pos, w, want_next=False)
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

    t_loop, t_wide = best_of(loop), best_of(wide)
    print(f"64 sequences, 7B shape, pos < 32: four l2z_transformer_batch calls {t_loop:.2f} ms, one l2z_transformer_wide "
          f"call {t_wide:.2f} ms ({t_loop / t_wide:.2f} x)")
    assert t_wide < t_loop
    for s in states:
        s.close()
    w.close()
