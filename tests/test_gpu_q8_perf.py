"""The int8 group-quantized decode against the f32 decode at the 7B width: two layers of
(4096, 11008, 32 heads, 32000, 256) at group size 64, the quantized weights built on the device from synthetic f32 ones.
The median of 7 readings of 32 stepped positions each; gated on "not slower" like the sibling perf tests, the figure is
printed (profiles/q8_bench.md has the full-depth numbers)."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SHAPE = (4096, 11008, 2, 32, 32, 32000, 256)
GS = 64
N_STEPS = 32
READINGS = 7


def median_ms_per_step(s, w):
    def reading():
        s.greedy_begin([])
        t0 = time.perf_counter()
        ids = s.greedy_run(w, N_STEPS)   # (returns after the ids are on the host)
        dt = time.perf_counter() - t0
        return dt, len(ids)
    reading()   # captures the graphs
    out = []
    for _ in range(READINGS):
        dt, n = reading()
        out.append(1e3 * dt / max(n, 1))
    return float(np.median(out))


def test_q8_step_is_not_slower_than_the_f32_step_at_the_7b_width(gpu, ck):
    cfg = ck.Config(*SHAPE)
    w32 = gpu.Weights(cfg, None, True, seed=5)
    w8 = gpu.Weights.quantized(w32, GS)
    s32, s8 = gpu.RunState(cfg), gpu.RunState(cfg)
    ms32 = median_ms_per_step(s32, w32)
    ms8 = median_ms_per_step(s8, w8)
    print(f"7B width, 2 layers: f32 {ms32:.4f} ms a step, q8 {ms8:.4f} ms a step, ratio {ms32 / ms8:.2f}")
    for x in (s32, s8, w32, w8):
        x.close()
    assert ms32 / ms8 >= 1.0
