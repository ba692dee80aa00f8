"""The batched prompt pass on int8 group-quantized weights (l2z_prefill_q8) on the GPU: its row launch bit
for bit against the activation rule, its GEMM on the int8 matrix cores against the product's derived bound, the whole pass
and its splits and hand-overs against tests/ref_q8.py, and the refusals.  tests/test_q8_prefill_cpu.py checks on the CPU
what these rely on; tests/q8_prefill_cases.py holds the shared inputs, tests/q8_cases.py the two bars."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cases  # noqa: E402
import q8_prefill_cases as pc  # noqa: E402
import ref_q8  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------- 1. the row launch, exact
@pytest.mark.parametrize("n,gs", [(64, 32), (64, 64), (288, 32), (4096, 32), (4096, 64), (11008, 32), (11008, 64)])
@pytest.mark.parametrize("m", [1, 15, 17])
def test_rows_launch_is_the_activation_rule_bit_for_bit(gpu, m, n, gs):
    x = pc.hard_rows(m, n, gs)
    q_ref, s_ref = ref_q8.quantize_act(x.reshape(-1), gs)
    if n // gs >= 5 or m >= 5:
        assert s_ref.min() == 0 and np.any((s_ref > 0) & (s_ref < 1e-38)), "the rows hold a zero and a denormal group"
    q, s = gpu.q8_quantize_rows(x, gs)
    np.testing.assert_array_equal(bits(s).reshape(-1), bits(s_ref))
    np.testing.assert_array_equal(q.reshape(-1), q_ref)


@pytest.mark.parametrize("n,gs", pc.NORM_CASES)
@pytest.mark.parametrize("m", [1, 17])
def test_rows_launch_with_the_norm_gives_the_reference_s_integers_and_scales(gpu, m, n, gs):
    """Inputs whose sum of squares is exact in f32 in any order and whose quotients keep their distance from every rounding
    boundary (tests/q8_prefill_cases.py, asserted in tests/test_q8_prefill_cpu.py): the launch's factor is three correctly
    rounded f32 operations on one exact number, so numpy's f32 gives its bits."""
    x, rms_w = pc.norm_rows(m, n, gs)
    q_ref, s_ref, _ = pc.norm_reference(x, rms_w, gs)
    q, s = gpu.q8_quantize_rows(x, gs, rms_w)
    print(f"m {m} n {n} gs {gs}: {int(np.sum(q != q_ref))} integers and {int(np.sum(bits(s) != bits(s_ref)))} scales differ")
    np.testing.assert_array_equal(q, q_ref)
    np.testing.assert_array_equal(bits(s), bits(s_ref))


# ---------------------------------------------------------------- 2. the GEMM, derived bound
# every m, d and (n, gs) of the list at least once; d = 4 and 36: a row tile of 16 that is not full
GEMM_CASES = [(1, 4, 64, 32), (15, 36, 288, 32), (16, 100, 768, 64), (17, 288, 4224, 64), (33, 2816, 288, 32),
              (100, 100, 11008, 32), (33, 36, 11008, 64), (17, 4, 4224, 64), (100, 288, 768, 64)]


def gemm_inputs(m, d, n, gs, fill):
    rng = np.random.default_rng(m * 11 + n * 7 + d * 3 + gs)
    if fill == "random":
        wq = rng.integers(-127, 128, (d, n)).astype(np.int8)
        xq = rng.integers(-127, 128, (m, n)).astype(np.int8)
    else:   # +-127 everywhere, and one weight row equal to a token row: |I| = gs * 127^2 in every group
        wq = np.where(rng.integers(0, 2, (d, n)) > 0, 127, -127).astype(np.int8)
        xq = np.where(rng.integers(0, 2, (m, n)) > 0, 127, -127).astype(np.int8)
        wq[d - 1] = xq[m - 1]
        if d > 1:
            wq[0] = -xq[0]
    ws = (rng.random((d, n // gs)) * 0.02 + 1e-4).astype(f32)
    xs = (rng.random((m, n // gs)) * 0.05 + 1e-4).astype(f32)
    return xq, xs, wq, ws


@pytest.mark.parametrize("m,d,n,gs", GEMM_CASES)
@pytest.mark.parametrize("fill", ["random", "extreme"])
def test_gemm_meets_the_derived_bound(gpu, m, d, n, gs, fill):
    """Per token row against the float64 value of sum_g f32(I) * ws * xs with the exact integer sums: two roundings a term
    and any order of the f32 sum stay within (G + 3) * 2^-24 * sum_g |term_g|, G = n / gs (tests/test_gpu_q8.py's bound)."""
    xq, xs, wq, ws = gemm_inputs(m, d, n, gs, fill)
    got = gpu.q8_gemm(xq, xs, wq, ws, gs)
    G = n // gs
    worst = 0.0
    for t in range(m):
        terms = ref_q8.matvec_terms64(wq, ws, xq[t], xs[t], gs)
        err = np.abs(got[t].astype(np.float64) - terms.sum(axis=1))
        bound = (G + 3) * 2.0 ** -24 * np.abs(terms).sum(axis=1)
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), f"token {t}: features over the bound: {np.flatnonzero(err > bound)[:8]}"
    print(f"m {m} d {d} n {n} gs {gs} {fill}: worst error / bound {worst:.3f}")
    if fill == "extreme":
        assert np.all(np.abs(ref_q8.group_sums(wq[d - 1:], xq[m - 1], gs)) == gs * 127 * 127)
    # the same bits on a second run
    np.testing.assert_array_equal(bits(gpu.q8_gemm(xq, xs, wq, ws, gs)), bits(got))
    # ... and a row's bits do not change when the other rows of the call are replaced, or leave
    keep = m // 2
    xq2, xs2, _, _ = gemm_inputs(m, d, n, gs, "random" if fill == "extreme" else "extreme")
    xq2[keep], xs2[keep] = xq[keep], xs[keep]
    np.testing.assert_array_equal(bits(gpu.q8_gemm(xq2, xs2, wq, ws, gs)[keep]), bits(got[keep]))
    np.testing.assert_array_equal(bits(gpu.q8_gemm(xq[keep:keep + 1], xs[keep:keep + 1], wq, ws, gs)[0]), bits(got[keep]))


# ---------------------------------------------------------------- 3. the whole pass
_flips = {}   # whole-pass case -> whether a position left the parity bar (the file's last test holds the tally)


def read_kv(s, cfg, P):
    L, S, kvd = cfg.n_layers, cfg.seq_len, cfg.kv_dim
    k = np.stack([s.read("key_cache", l * S * kvd, P * kvd).reshape(P, kvd) for l in range(L)])
    v = np.stack([s.read("value_cache", l * S * kvd, P * kvd).reshape(P, kvd) for l in range(L)])
    return k, v


def run_device(gpu, name, w):
    """prefill_q8 of the whole run: its K / V rows and last logits; and of every prefix on a fresh runstate: position p's
    logits (the last layer's Wo / W1 | W3 / W2 of every row reach only these)."""
    cfg = q8_cases.model(name)[0]
    toks = pc.tokens(name)
    s = gpu.RunState(cfg)
    s.prefill_q8(toks, 0, w)
    k, v = read_kv(s, cfg, toks.size)
    z = {toks.size - 1: s.logits()}
    tok = s.argmax()
    s.close()
    assert tok == int(np.argmax(z[toks.size - 1]))   # (the classifier's candidates, as after a decode step)
    for p in range(toks.size - 1):
        s = gpu.RunState(cfg)
        s.prefill_q8(toks[:p + 1], 0, w)
        z[p] = s.logits()
        s.close()
    return z, k, v


@pytest.mark.parametrize("name", list(pc.RUN_LENGTH))
def test_whole_pass_against_the_float64_reference(gpu, name):
    cfg, gs, _, body = q8_cases.model(name)
    w = gpu.Weights.from_q8(cfg, body, True, gs)
    z, k, v = run_device(gpu, name, w)
    flipped, ok, dev = pc.check_rule(z, k, v, pc.reference(name, "f64"))
    print(f"shape {name}: positions over the parity bar {list(np.flatnonzero(~ok))}, largest deviation {dev.max():.3e} of the scale")
    _flips[name] = flipped
    z2, k2, v2 = run_device(gpu, name, w)   # the same bits from run to run
    for p in z:
        np.testing.assert_array_equal(bits(z[p]), bits(z2[p]))
    np.testing.assert_array_equal(bits(k), bits(k2))
    np.testing.assert_array_equal(bits(v), bits(v2))
    w.close()


# ---------------------------------------------------------------- 4. splits and hand-overs
@pytest.mark.parametrize("name", ["64", "512"])
def test_a_prompt_in_two_calls_meets_the_reference(gpu, name):
    cfg, gs, _, body = q8_cases.model(name)
    w = gpu.Weights.from_q8(cfg, body, True, gs)
    toks = pc.tokens(name)
    s = gpu.RunState(cfg)
    s.prefill_q8(toks[:5], 0, w)
    z = {4: s.logits()}
    s.prefill_q8(toks[5:], 5, w)
    z[toks.size - 1] = s.logits()
    k, v = read_kv(s, cfg, toks.size)
    flipped, ok, dev = pc.check_rule(z, k, v, pc.reference(name, "f64"))
    print(f"shape {name}, 5 + {toks.size - 5}: positions over the parity bar {list(np.flatnonzero(~ok))}, largest deviation {dev.max():.3e}")
    s.close(); w.close()


@pytest.mark.parametrize("name", ["64", "512"])
def test_transformer_steps_continue_from_the_prompt_pass(gpu, name):
    cfg, gs, _, body = q8_cases.model(name)
    w = gpu.Weights.from_q8(cfg, body, True, gs)
    toks = pc.tokens(name)
    half = toks.size // 2
    s = gpu.RunState(cfg)
    s.prefill_q8(toks[:half], 0, w)
    z = {half - 1: s.logits()}
    for p in range(half, toks.size):
        s.transformer(int(toks[p]), p, w)
        z[p] = s.logits()
    k, v = read_kv(s, cfg, toks.size)
    flipped, ok, dev = pc.check_rule(z, k, v, pc.reference(name, "f64"))
    print(f"shape {name}, {half} batched + {toks.size - half} stepped: positions over the parity bar {list(np.flatnonzero(~ok))}, "
          f"largest deviation {dev.max():.3e}")
    s.close(); w.close()


def test_generate_q8_emits_the_ids_of_the_reference(gpu):
    """The checkpoint built for the greedy loop (q8_cases.peaked_model): the reference's top-2 margin is at least 10 x the
    loose bar at every step -- no flipped activation can change an id --, so the prompt pass + stepped generation emits
    the reference's ids."""
    ids_ref, margins, zs = q8_cases.peaked_reference()
    scale = np.abs(zs).max(axis=1)
    assert np.all(margins >= 10 * q8_cases.LOOSE * scale)
    assert 1 not in ids_ref and list(ids_ref[:5]) == q8_cases.GREEDY_PROMPT
    cfg, gs, body = q8_cases.peaked_model()
    w = gpu.Weights.from_q8(cfg, body, False, gs)
    s = gpu.RunState(cfg)
    ids = gpu.generate_q8(s, w, q8_cases.GREEDY_PROMPT, q8_cases.GREEDY_STEPS)
    np.testing.assert_array_equal(ids, ids_ref)
    assert q8_cases.parity_ok(s.logits(), zs[-1]) or q8_cases.scaled_dev(s.logits(), zs[-1]) <= q8_cases.LOOSE
    s.close(); w.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_enqueue_nothing_and_change_nothing(gpu):
    B = gpu
    cfg, gs, blob, body = q8_cases.model("64")
    w = B.Weights.from_q8(cfg, body, True, gs)
    w32 = B.Weights(cfg, blob, True)
    toks = pc.tokens("64")
    s, twin = B.RunState(cfg), B.RunState(cfg)
    for r in (s, twin):
        r.prefill_q8(toks[:7], 0, w)
    S, kvd, V = cfg.seq_len, cfg.kv_dim, cfg.vocab_size

    def sampled():
        return (s.logits(), s.read("key_cache", (S + 4) * kvd, kvd), s.read("value_cache", 2 * kvd, kvd),
                s.read("key_cache", 7 * kvd, 2 * kvd), s.read("value_cache", (S + 7) * kvd, 2 * kvd))

    before = sampled()
    pool = B.KvPool(cfg, 4)
    sp = B.RunState(cfg, pool=pool)
    comm = B.Comm(0, 2, None, 0, emulated=True)
    ss = B.RunState(cfg, comm=comm)
    three = [7, 8, 9]
    calls = {
        "f32 weights": (lambda: s.prefill_q8(three, 7, w32), B.ERR_INVALID, "l2z_prefill"),
        "a paged runstate": (lambda: sp.prefill_q8(three, 0, w), B.ERR_INVALID, ""),
        "a sharded runstate": (lambda: ss.prefill_q8(three, 0, w), B.ERR_INVALID, ""),
        "positions past seq_len": (lambda: s.prefill_q8(three, S - 2, w), B.ERR_STATE, ""),
        "a negative position": (lambda: s.prefill_q8(three, -1, w), B.ERR_STATE, ""),
        "token = vocab_size": (lambda: s.prefill_q8([7, V, 9], 7, w), B.ERR_STATE, ""),
        "n_tokens = 0": (lambda: s.prefill_q8([], 7, w), B.ERR_INVALID, ""),
    }
    for what, (call, code, word) in calls.items():
        with pytest.raises(B.L2ZError) as e:
            call()
        assert e.value.code == code, f"{what}: {e.value}"
        assert word in str(e.value), f"{what}: {e.value}"
    for a, b in zip(before, sampled()):
        np.testing.assert_array_equal(bits(a), bits(b))
    # ... and the next position: the sequence goes on exactly as its undisturbed twin's
    for r in (s, twin):
        r.transformer(int(toks[7]), 7, w)
    np.testing.assert_array_equal(bits(s.logits()), bits(twin.logits()))
    assert s.argmax() == twin.argmax()
    # the existing prompt pass still refuses such weights
    with pytest.raises(B.L2ZError) as e:
        s.prefill(three, 8, w)
    assert e.value.code == B.ERR_INVALID
    sp.close(); pool.close(); ss.close(); comm.close()
    for r in (s, twin):
        r.close()
    w.close(); w32.close()


# ---------------------------------------------------------------- the tally (keep this test last)
def test_at_most_one_whole_pass_case_left_the_parity_bar():
    """A flipped activation -- a position over the parity bar and under the loose one -- in at most one of the whole-pass
    cases that ran: the two CPU modes need none (tests/test_q8_prefill_cpu.py), and the decode pass needed none."""
    flipped = [name for name, f in _flips.items() if f]
    print(f"whole-pass cases run: {sorted(_flips)}, with a position over the parity bar: {flipped}")
    assert len(flipped) <= 1
