"""What tests/test_gpu_q8_prefill.py relies on, checked where it is cheap (no GPU): on every token run the batched pass's
tests use (tests/q8_prefill_cases.py), the two arithmetic modes of tests/ref_q8.py agree within the project's parity bar at
EVERY position -- an exception on the device is then the device's summation order alone --, and the row launch's inputs
with the norm keep their margin, so the numpy reference's integers are the only correct ones."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cases  # noqa: E402
import q8_kernel_cases  # noqa: E402
import q8_prefill_cases as pc  # noqa: E402
import ref_q8  # noqa: E402


def test_the_runs_extend_the_decode_tests_tokens():
    assert pc.RUN_LENGTH == {"64": 32, "288": 12, "512": 24, "tall": 12}
    for name, n in pc.RUN_LENGTH.items():
        toks = pc.tokens(name)
        cfg = q8_cases.model(name)[0]
        assert toks.size == n <= cfg.seq_len and toks.min() >= 2 and toks.max() < cfg.vocab_size
        np.testing.assert_array_equal(toks[:q8_cases.N_POS], q8_cases.tokens(name))
    # more than one token tile of 16 in one chunk, and a last tile that is not full
    assert pc.RUN_LENGTH["64"] == 2 * 16 and pc.RUN_LENGTH["512"] % 16 == 8


@pytest.mark.parametrize("name", list(pc.RUN_LENGTH))
def test_the_two_modes_agree_on_every_run_without_an_exception(name):
    z32, k32, v32, _ = pc.reference(name, "f32")
    ref = pc.reference(name, "f64")
    flipped, ok, dev = pc.check_rule({p: z32[p] for p in range(z32.shape[0])}, k32, v32, ref)
    print(f"shape {name}: {z32.shape[0]} positions, largest deviation between the modes {dev.max():.3e} of the scale, "
          f"smallest quantization margin {ref[3]:.3e} of a step")
    assert not flipped and ok.all() and dev.max() < 1e-5
    if name in ("288", "tall"):   # the twelve-position runs are q8_cases' own
        np.testing.assert_array_equal(ref[0], q8_cases.reference(name, "f64")[0])


@pytest.mark.parametrize("n,gs", pc.NORM_CASES)
def test_the_row_launch_s_normed_inputs_keep_their_margin(n, gs):
    """The f32 statement-by-statement reference quantizes to the float64 reference's integers (the only correct ones:
    tests/test_ref_q8_cpu.py), every quotient at least 2^-11 from a rounding boundary; negating a row negates its integers
    and keeps its scales."""
    x, rms_w = pc.norm_rows(3, n, gs)
    q, s, margin = pc.norm_reference(x, rms_w, gs)
    xq, xs, _, _ = q8_kernel_cases.prologue_reference(n, gs, True)
    print(f"n {n} gs {gs}: smallest distance of a quotient to a boundary {margin:.3e}")
    assert margin >= q8_kernel_cases.MARGIN / 2
    np.testing.assert_array_equal(q[0], xq)
    np.testing.assert_array_equal(q[1], -xq)
    np.testing.assert_array_equal(q[2], xq)
    assert np.array_equal(s[0].view(np.uint32), s[1].view(np.uint32)) and np.all(s > 0)
    assert np.max(np.abs(s[0].astype(np.float64) / xs - 1)) < 4 * 2.0 ** -24   # (the float64 factor's scales: a few ulp off)


def test_the_hard_rows_hold_every_kind_of_group():
    for n, gs in ((64, 32), (288, 32), (4096, 64)):
        x = pc.hard_rows(5, n, gs)
        q, s = ref_q8.quantize_act(x.reshape(-1), gs)
        assert s.min() == 0 and np.any((s > 0) & (s < 1e-38)) and np.abs(q).max() == 127
        assert not np.array_equal(x[0], x[1])
