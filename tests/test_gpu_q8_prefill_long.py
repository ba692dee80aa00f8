"""The batched prompt pass on int8 group-quantized weights (l2z_prefill_q8) past 128 rows, on the GPU: the
GEMM where a launch has more than one column of blocks, and the whole pass on prompts of up to 600 tokens -- chunks of
several columns, the chunk loop inside one call, the scratch's grow rule.  (The residual and SwiGLU epilogues of the GEMM
are still reached through the whole pass only.)

The pass is discontinuous, so a long run against tests/ref_q8.py is fragile (one such run is here, on a swept seed); what
holds the new rows are EXACT relations to paths tests/test_gpu_q8_prefill.py already pins to float64: a row of the GEMM has
the bits of the same row in a call of at most 16 rows, and on the two shapes of tests/q8_prefill_long_cases.py -- whose
attention stays on the block-per-(head, query) kernel -- the whole pass has the same bits however the prompt is cut into
chunks and calls.  No tolerance is involved in those.  tests/test_q8_prefill_long_cpu.py checks on the CPU what this file
relies on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cases  # noqa: E402
import q8_prefill_cases as pc  # noqa: E402
import q8_prefill_long_cases as lc  # noqa: E402
import ref_q8  # noqa: E402
from test_gpu_q8_prefill import gemm_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def assert_rows_equal(got, want, what):
    """Bit for bit, naming the rows that differ."""
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, f"{what}: shapes {got.shape} and {want.shape}"
    rows = np.flatnonzero(np.any(got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1), axis=1))
    assert rows.size == 0, f"{what}: {rows.size} rows differ, the first {list(rows[:12])}"
    np.testing.assert_array_equal(got, want)


def by_row_tiles(m, call):
    """The rows of `call(slice)` over calls of at most 16 rows, stacked."""
    return np.concatenate([call(sl) for sl in lc.row_slices(m)], axis=0)


# ---------------------------------------------------------------- 1. the GEMM past one column of blocks
@pytest.mark.parametrize("m,d,n,gs", list(lc.GEMM_LONG_CASES))
@pytest.mark.parametrize("fill", ["random", "extreme"])
def test_gemm_past_one_column_meets_the_bound_and_every_row_has_its_short_call_s_bits(gpu, m, d, n, gs, fill):
    """The derived bound of test_gemm_meets_the_derived_bound, per token row against ref_q8.matvec_terms64; and every row
    bit for bit the same row of a call of at most 16 rows -- the one-tile path the existing cases pin --, so a wrong
    tile, column or row offset anywhere in the grid is a bit difference in a named row."""
    n_tiles, nt, n_tt, last, row_tiles, live = lc.gemm_grid(m, d)
    assert nt == lc.NT_MAX and n_tt > 1 and (n_tt, last) == lc.GEMM_LONG_CASES[(m, d, n, gs)]
    xq, xs, wq, ws = gemm_inputs(m, d, n, gs, fill)
    got = gpu.q8_gemm(xq, xs, wq, ws, gs)
    G = n // gs
    worst, over = 0.0, []
    for t in range(m):
        terms = ref_q8.matvec_terms64(wq, ws, xq[t], xs[t], gs)
        err = np.abs(got[t].astype(np.float64) - terms.sum(axis=1))
        bound = (G + 3) * 2.0 ** -24 * np.abs(terms).sum(axis=1)
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        if np.any(err > bound):
            over.append(t)
    print(f"m {m} d {d} n {n} gs {gs} {fill}: {n_tt} columns, {last} tiles in the last, {row_tiles} row tiles: "
          f"worst error / bound {worst:.3f}")
    assert not over, f"{len(over)} token rows over the bound, the first {over[:12]}"
    if fill == "extreme":
        assert np.all(np.abs(ref_q8.group_sums(wq[d - 1:], xq[m - 1], gs)) == gs * 127 * 127)
    assert_rows_equal(got, by_row_tiles(m, lambda sl: gpu.q8_gemm(xq[sl], xs[sl], wq, ws, gs)), "against calls of at most 16 rows")
    np.testing.assert_array_equal(bits(gpu.q8_gemm(xq, xs, wq, ws, gs)), bits(got))   # the same bits on a second run


# ---------------------------------------------------------------- 2. the whole pass on long prompts
def read_kv(s, cfg, P):
    L, S, kvd = cfg.n_layers, cfg.seq_len, cfg.kv_dim
    k = np.stack([s.read("key_cache", l * S * kvd, P * kvd).reshape(P, kvd) for l in range(L)])
    v = np.stack([s.read("value_cache", l * S * kvd, P * kvd).reshape(P, kvd) for l in range(L)])
    return k, v


def feed(s, w, toks, calls, pos0=0):
    """toks in calls of the given lengths at consecutive positions"""
    assert sum(calls) == len(toks)
    at = 0
    for n in calls:
        s.prefill_q8(toks[at:at + n], pos0 + at, w)
        at += n


def state(s, cfg, P):
    k, v = read_kv(s, cfg, P)
    return {"K rows": k.transpose(1, 0, 2), "V rows": v.transpose(1, 0, 2), "logits": s.logits()[None, :],
            "argmax": np.array([[s.argmax()]], f32)}   # (position-major, so that a difference names its position)


def assert_same_state(a, b, what):
    for key in a:
        assert_rows_equal(a[key], b[key], f"{what}: {key}")


def open_model(gpu, name, gs=None):
    cfg, gs, _, body = lc.model(name, gs=gs)
    return cfg, gpu.Weights.from_q8(cfg, body, True, gs)


def two_ways(gpu, options, name, plan_one, plan_many):
    """Two fresh runstates fed the same tokens by two plans of lc.CHUNK_PLANS, the knob set before each."""
    cfg, w = open_model(gpu, name)
    (chunk_a, calls_a), (chunk_b, calls_b) = lc.CHUNK_PLANS[plan_one], lc.CHUNK_PLANS[plan_many]
    P = sum(calls_a)
    assert P == sum(calls_b)
    toks = lc.tokens(name, P)
    sa, sb = gpu.RunState(cfg), gpu.RunState(cfg)
    options(L2Z_PF_CHUNK=chunk_a)
    feed(sa, w, toks, calls_a)
    options(L2Z_PF_CHUNK=chunk_b)
    feed(sb, w, toks, calls_b)
    return cfg, w, sa, sb, P


@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_a_one_chunk_of_300_rows_equals_calls_of_at_most_128(gpu, options, name):
    """One chunk of three columns of blocks against calls of 128, 128 and 44 at positions 0, 128 and 256 -- chunks of one
    column, two calls, the path tests/test_gpu_q8_prefill.py covers."""
    cfg, w, one, many, P = two_ways(gpu, options, name, "a one chunk", "a calls of 128")
    assert_same_state(state(one, cfg, P), state(many, cfg, P), f"{name}, one chunk of {P} against calls of 128, 128, 44")
    one.close(); many.close(); w.close()


@pytest.mark.parametrize("plan", ["b 144", "b 48"])
@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_b_the_chunk_loop_inside_a_call_equals_separate_calls(gpu, options, name, plan):
    """tokens + done, pos0 + done and the hand-over of the LAST chunk's last row to the classifier: one call of three
    chunks against three calls of those lengths at those positions."""
    one_plan, many_plan = plan + " in one call", plan + " as calls"
    chunk, (n_tokens,) = lc.CHUNK_PLANS[one_plan][0], lc.CHUNK_PLANS[one_plan][1]
    assert lc.chunks_of(chunk, n_tokens) == lc.CHUNK_PLANS[many_plan][1] and len(lc.CHUNK_PLANS[many_plan][1]) == 3
    cfg, w, one, many, P = two_ways(gpu, options, name, one_plan, many_plan)
    assert_same_state(state(one, cfg, P), state(many, cfg, P), f"{name}, L2Z_PF_CHUNK {chunk} on {P} tokens")
    one.close(); many.close(); w.close()


@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_c_the_scratch_grows_and_stays_without_a_trace(gpu, options, name):
    """q8pf_alloc: 20 rows make the scratch at 512, 600 rows in one chunk re-make it at 1024, 20 rows again find it large
    enough.  At each step the runstate equals a fresh one given that step's call alone, and the rows a step does not write
    are still the step's before."""
    chunk, (first, grown, again) = lc.CHUNK_PLANS["c grow"]
    assert first <= 512 < grown <= 1024 and lc.chunks_of(chunk, grown) == [grown] and again <= 512
    options(L2Z_PF_CHUNK=chunk)
    cfg, w = open_model(gpu, name)
    toks = lc.tokens(name, cfg.seq_len)
    steps = [toks[:first], toks[:grown], toks[grown:grown + again]]   # all from position 0; the last on other tokens
    a = gpu.RunState(cfg)
    before = None
    for i, run in enumerate(steps):
        a.prefill_q8(run, 0, w)
        fresh = gpu.RunState(cfg)
        fresh.prefill_q8(run, 0, w)
        got = state(a, cfg, run.size)
        assert_same_state(got, state(fresh, cfg, run.size), f"{name}, step {i} ({run.size} tokens)")
        fresh.close()
        if before is not None and run.size < before["K rows"].shape[0]:
            kept = state(a, cfg, before["K rows"].shape[0])
            for key in ("K rows", "V rows"):
                assert_rows_equal(kept[key][run.size:], before[key][run.size:], f"{name}, step {i}: {key} the step does not write")
        before = got
    a.close(); w.close()


def test_c_the_scratch_is_made_again_for_another_group_size(gpu, options):
    """One runstate with GS-32, then GS-64, then GS-32 weights of one checkpoint (the scale rows of the scratch are twice
    as long at 32): each call equals a fresh runstate's."""
    options(L2Z_PF_CHUNK=2048)
    name, P = "long64", 100
    toks = lc.tokens(name, P)
    models = {gs: open_model(gpu, name, gs) for gs in (32, 64)}
    cfg = models[32][0]
    a = gpu.RunState(cfg)
    logits = {}
    for i, gs in enumerate((32, 64, 32)):
        w = models[gs][1]
        a.prefill_q8(toks, 0, w)
        fresh = gpu.RunState(cfg)
        fresh.prefill_q8(toks, 0, w)
        assert_same_state(state(a, cfg, P), state(fresh, cfg, P), f"call {i}, group size {gs}")
        fresh.close()
        logits[gs] = a.logits()
    assert np.any(bits(logits[32]) != bits(logits[64]))   # (the two quantizations are two models)
    a.close()
    for _, w in models.values():
        w.close()


def test_d_300_tokens_in_one_chunk_against_the_float64_reference(gpu, options):
    """"long64" on its swept seed (tests/q8_prefill_long_cases.py SWEEP): K and V rows at all 300 positions, the logits at
    the positions around the column and tile boundaries, each the last of a prefix on a fresh runstate; q8_prefill_cases'
    rule and q8_cases' bars unchanged.  What holds rows 128 and above conclusively is a to c above, not this run."""
    chunk, (P,) = lc.CHUNK_PLANS["d reference"]
    assert P == lc.REF_TOKENS and max(lc.REF_LOGIT_POSITIONS) == P - 1
    options(L2Z_PF_CHUNK=chunk)
    cfg, w = open_model(gpu, "long64")
    toks = lc.tokens("long64", P)
    z = {}
    for p in lc.REF_LOGIT_POSITIONS:
        s = gpu.RunState(cfg)
        s.prefill_q8(toks[:p + 1], 0, w)
        z[p] = s.logits()
        if p == P - 1:
            k, v = read_kv(s, cfg, P)
            assert s.argmax() == int(np.argmax(z[p]))
        s.close()
    flipped, ok, dev = pc.check_rule(z, k, v, lc.reference("f64"))
    print(f"long64, {P} tokens in one chunk: a position left the parity bar: {flipped} {list(np.flatnonzero(~ok))[:8]}, "
          f"largest deviation {dev.max():.3e} of the scale (the loose bar: {q8_cases.LOOSE})")
    w.close()


@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_e_a_transformer_step_goes_on_from_either_cut(gpu, options, name):
    cfg, w, one, many, P = two_ways(gpu, options, name, "a one chunk", "a calls of 128")
    tok = int(lc.tokens(name, P + 1)[P])
    for s in (one, many):
        s.transformer(tok, P, w)
    assert_same_state(state(one, cfg, P + 1), state(many, cfg, P + 1), f"{name}, the step at position {P}")
    one.close(); many.close(); w.close()


@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_e_generate_q8_on_a_long_prompt_emits_the_ids_of_the_cut_prompt(gpu, options, name):
    """BOS + 139 tokens, 140 positions in one call of generate_q8, against calls of 128 and 12 and the same stepped loop."""
    (chunk, (P,)), (_, calls) = lc.CHUNK_PLANS["e generate"], lc.CHUNK_PLANS["e generate as calls"]
    options(L2Z_PF_CHUNK=chunk)
    cfg, w = open_model(gpu, name)
    prompt = [int(t) for t in lc.tokens(name, P - 1)]
    steps = P + 24
    s = gpu.RunState(cfg)
    ids = gpu.generate_q8(s, w, prompt, steps)
    s2 = gpu.RunState(cfg)
    feed(s2, w, np.array([1] + prompt, np.int32), calls)
    want = list(prompt)
    tok = s2.argmax()
    want.append(tok)
    for pos in range(P, steps):
        if tok == 1:
            break
        s2.transformer(tok, pos, w)
        tok = s2.argmax()
        want.append(tok)
    assert len(want) > P or want[-1] == 1
    np.testing.assert_array_equal(ids, np.array(want, np.int32))
    np.testing.assert_array_equal(bits(s.logits()), bits(s2.logits()))
    s.close(); s2.close(); w.close()
