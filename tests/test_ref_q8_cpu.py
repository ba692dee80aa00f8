"""What the GPU tests of the int8 group-quantized pass rely on, checked where it is cheap (no GPU): the two arithmetic
modes of tests/ref_q8.py -- f32 in runq.c's sequential order, and float64 -- agree within the project's parity bar
(5e-5 + 5e-5 |x|) on the GPU tests' own inputs, at EVERY position: the one exception the whole-pass rule allows is then for
the device's summation order alone.  Also the reference's own pieces against hand-computed values."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cases  # noqa: E402
import q8_kernel_cases  # noqa: E402
import ref_q8  # noqa: E402

f32 = np.float32


@pytest.mark.parametrize("name", list(q8_cases.SHAPES))
def test_the_two_modes_agree_on_the_gpu_tests_inputs_without_an_exception(name):
    z32, k32, v32 = q8_cases.reference(name, "f32")
    ok, dev = q8_cases.check_positions(z32, k32, v32, *q8_cases.reference(name, "f64"), exceptions=0)
    print(f"shape {name}: largest deviation between the modes {dev.max():.3e} of the scale")
    assert ok.all() and dev.max() < 1e-5


def test_the_loose_bar_is_four_times_the_measured_deviation():
    """scripts/q8_loose_bar.py's sweep (756 positions) gave 0.0275 of the scale; a flipped case of that
    sweep, re-run here, lies above the parity bar and under the measured figure."""
    assert q8_cases.LOOSE == 4 * 0.0275
    import __graft_entry__ as ge
    ck = ge.load_package().checkpoint
    cfg, gs, _, body = q8_cases.model("288", 100)
    toks = q8_cases.tokens("288", 100)
    z32, m32 = ref_q8.run_positions(ck, cfg, body, True, gs, toks, "f32")
    z64, m64 = ref_q8.run_positions(ck, cfg, body, True, gs, toks, "f64")
    P = q8_cases.N_POS
    ok, dev = q8_cases.position_report(z32, m32.kc[:, :P], m32.vc[:, :P], z64, m64.kc[:, :P], m64.vc[:, :P])
    assert not ok.all() and 1e-4 < dev.max() <= q8_cases.LOOSE_MEASURED


def test_the_greedy_checkpoint_has_margins_of_ten_loose_bars():
    """tests/test_gpu_q8.py's greedy test relies on it: both modes emit the same ids, the walk t -> NEXT[t]."""
    import __graft_entry__ as ge
    ids, margins, zs = q8_cases.peaked_reference()
    assert np.all(margins >= 10 * q8_cases.LOOSE * np.abs(zs).max(axis=1))
    walk = list(q8_cases.GREEDY_PROMPT)
    while len(walk) < q8_cases.GREEDY_STEPS:
        walk.append(int(q8_cases.NEXT[walk[-1]]))
    assert ids.tolist() == walk
    cfg, gs, body = q8_cases.peaked_model()
    ids32, _, _ = ref_q8.greedy(ge.load_package().checkpoint, cfg, body, False, gs, q8_cases.GREEDY_PROMPT, q8_cases.GREEDY_STEPS, "f32")
    assert ids32.tolist() == walk


def test_activation_rule_rounds_half_away_from_zero_from_the_f32_quotient():
    v = np.zeros(32, f32)
    v[:10] = np.array([127, 0.5, -0.5, 1.5, -1.5, 2.5, 126.5, -126.5, 0.49999997, -0.49999997], f32) * f32(0.125)
    q, s = ref_q8.quantize_act(v, 32)
    assert s.tolist() == [0.125]
    assert q[:10].tolist() == [127, 1, -1, 2, -2, 3, 127, -127, 0, 0]   # floor(|v| + 0.5) in f32 would give 1 for 0.49999997
    q, s = ref_q8.quantize_act(np.zeros(64, f32), 32)
    assert s.tolist() == [0, 0] and not q.any()


def test_matvec_modes_on_a_hand_computed_product():
    wq = np.array([[1] * 32 + [2] * 32, [-127] * 64], np.int8)
    xq = np.array([3] * 32 + [-1] * 32, np.int8)
    ws = np.array([[0.5, 0.25], [1.0, 2.0]], f32)
    xs = np.array([2.0, 4.0], f32)
    assert ref_q8.group_sums(wq, xq, 32).tolist() == [[96, -64], [-12192, 4064]]
    want = [96 * 0.5 * 2 - 64 * 0.25 * 4, -12192 * 1.0 * 2 + 4064 * 2.0 * 4]
    assert ref_q8.matvec(wq, ws, xq, xs, 32, "f64").tolist() == want
    assert ref_q8.matvec(wq, ws, xq, xs, 32, "f32").tolist() == want


@pytest.mark.parametrize("n,gs,norm", q8_kernel_cases.PROLOGUE_CASES)
def test_the_fused_prologues_inputs_keep_their_margin(n, gs, norm):
    """tests/test_gpu_q8_kernel.py's tight prologue test relies on it: the sum of squares is exact in f32 in any order, and
    with the norm every quotient of the reference lies at least 2^-10 from a rounding boundary -- a device factor a few
    ulp off moves a quotient of at most 127 by under 2^-15 --, so the reference's integers are the only correct ones."""
    x, rms_w, wq, ws = q8_kernel_cases.prologue_case(n, gs, norm)
    k = x.astype(np.float64) * 8
    assert np.array_equal(k, np.round(k)) and np.abs(k).max() <= 16
    exact = float(np.sum(x.astype(np.float64) ** 2))
    assert exact * 64 < 2 ** 24   # in units of 2^-6: every partial sum is an integer below 2^24
    rng = np.random.default_rng(n)
    for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):   # any order of the f32 sum gives it
        assert float(np.cumsum((x[order] * x[order]).astype(f32), dtype=f32)[-1]) == exact
    xq, xs, margin, terms = q8_kernel_cases.prologue_reference(n, gs, norm)
    print(f"n {n} gs {gs} norm {norm}: smallest distance of a quotient to a boundary {margin:.3e}")
    assert (xs > 0).all() and np.abs(xq).reshape(-1, gs).max(axis=1).min() == 127 and terms.shape == (wq.shape[0], n // gs)
    if norm:
        assert margin >= q8_kernel_cases.MARGIN
        # ... and a factor 8 ulp off either way quantizes to the same integers
        v = x.astype(np.float64) * (1.0 / np.sqrt(exact / n + 1e-5))
        for off in (1 - 2.0 ** -21, 1 + 2.0 ** -21):
            q2, s2 = ref_q8.quantize_act(((v * off) * rms_w.astype(np.float64)).astype(f32), gs)
            assert np.array_equal(q2, xq)
