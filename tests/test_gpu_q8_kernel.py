"""The int8 mat-vec kernel (q8_matvec.hip) driven as the pass drives it, one launch at a time, through
l2z_q8_matvec_case: rows wider than one batch of 4096 columns, several pairs a wave, every epilogue and the fused
rmsnorm + quantize prologue -- each held to what can be derived for it, not to the whole pass's loose bar.

Every case asserts the loop structure it was built for, from the grid the launcher reports:
    batches = ceil(n / 4096)                 (a lane holds 4 chunks of 16 bytes a batch: 64 * 4 * 16 columns)
    units_per_wave = ceil(n_pairs / (4 * grid))
so a case can never pass without taking the branch.

The epilogues are checked EXACTLY, given the store epilogue's output y on the same inputs as the device's sums: the sums
are functions of a row's contents, n and gs only.  tests/q8_kernel_cases.py builds the prologue's inputs and
tests/test_ref_q8_cpu.py checks their margins on the CPU.  profiles/q8_kernel_pins.md holds what the device gave."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_kernel_cases as kc  # noqa: E402
import ref_q8  # noqa: E402
from test_gpu_q8 import quantize_rows  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
BATCH = 64 * 4 * 16   # columns of one batch of a wave
ONE_BLOCK = dict(n_cus=1, max_blocks_per_cu=1)
THREE_BLOCKS = dict(n_cus=3, max_blocks_per_cu=1)
GRIDS = {"default": {}, "one": ONE_BLOCK, "three": THREE_BLOCKS}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def ceil_div(a, b):
    return -(-a // b)


def units_per_wave(res):
    return ceil_div(res["n_pairs"], 4 * res["grid"])


def expected_grid(n_pairs, which):
    """The launcher's grid where fewer blocks than are resident cover the pairs ("default", small cases), and under
    the two overrides: at most 1 or 3 blocks, the pairs dealt evenly."""
    g = ceil_div(n_pairs, 4)
    cap = {"default": g, "one": 1, "three": 3}[which]
    if g <= cap:
        return g
    per_wave = ceil_div(n_pairs, 4 * cap)
    return ceil_div(n_pairs, 4 * per_wave)


def check_bound(got, terms, extra, what):
    """|got - sum of the float64 terms| <= (G + extra) * 2^-24 * sum |term|; returns the worst error / bound"""
    ref = terms.sum(axis=1)
    bound = (terms.shape[1] + extra) * 2.0 ** -24 * np.abs(terms).sum(axis=1)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert np.all(err <= bound), f"{what}: rows over the bound {np.flatnonzero(err > bound)[:8]}, worst ratio {ratio:.3g}"
    return ratio


def weights(rng, rows, n, gs):
    return rng.integers(-127, 128, (rows, n)).astype(np.int8), (rng.random((rows, n // gs)) * 0.02 + 1e-4).astype(f32)


def quantized_x(rng, n, gs):
    return rng.integers(-127, 128, n).astype(np.int8), (rng.random(n // gs) * 0.05 + 1e-4).astype(f32)


def float_x(rng, n):
    return (rng.standard_normal(n) * 1.5).astype(f32), (rng.random(n) + 0.5).astype(f32)


# ---------------------------------------------------------------- a. several batches a row
def runs_past_the_first_batch(rng, wq, xq):
    """+-127 in runs of 16 columns past column 4096, of either operand: a chunk dropped or taken twice moves a sum by
    16 * 127 * 127 scaled, orders of magnitude above the bound"""
    n = xq.size
    runs = (n - BATCH) // 16
    xq[BATCH:] = np.repeat(np.where(rng.integers(0, 2, runs) > 0, 127, -127), 16)
    wq[:, BATCH:] = np.repeat(np.where(rng.integers(0, 2, (wq.shape[0], runs)) > 0, 127, -127), 16, axis=1)


@pytest.mark.parametrize("d", [7, 24])
@pytest.mark.parametrize("n,gs", [(4128, 32), (4160, 64), (8192, 32), (8192, 64), (11008, 32), (11008, 64)])
def test_rows_of_several_batches_meet_the_derived_bound(gpu, n, gs, d):
    """A two-lane (gs 32) and a four-lane (gs 64) second batch, exactly two full batches, and W2's width at 7B; the
    store epilogue on a quantized x against the float64 terms, (G + 3) * 2^-24 * sum |term| as in test_gpu_q8.py."""
    rng = np.random.default_rng(n * 11 + gs + d)
    wq, ws = weights(rng, d, n, gs)
    xq, xs = quantized_x(rng, n, gs)
    runs_past_the_first_batch(rng, wq, xq)
    res = gpu.q8_matvec_case("store", gs, [(wq, ws)], xq=xq, xs=xs)
    assert ceil_div(n, BATCH) == {4128: 2, 4160: 2, 8192: 2, 11008: 3}[n]
    assert res["grid"] == ceil_div(d, 8) and units_per_wave(res) == 1
    check_bound(res["outs"][0], ref_q8.matvec_terms64(wq, ws, xq, xs, gs), 3, f"n {n} gs {gs} d {d}")
    np.testing.assert_array_equal(bits(res["outs"][0]), bits(gpu.q8_matmul(xq, xs, wq, ws, gs)))


# ---------------------------------------------------------------- e. the launcher's branch for more than 64 KiB of LDS
def test_a_row_that_needs_more_than_64_kib_of_lds(gpu):
    n, gs, d = 65536, 32, 4
    assert n + (n // gs + 32) * 4 > 64 * 1024
    rng = np.random.default_rng(65536)
    wq, ws = weights(rng, d, n, gs)
    xq, xs = quantized_x(rng, n, gs)
    runs_past_the_first_batch(rng, wq, xq)
    res = gpu.q8_matvec_case("store", gs, [(wq, ws)], xq=xq, xs=xs)
    assert ceil_div(n, BATCH) == 16 and res["grid"] == 1
    check_bound(res["outs"][0], ref_q8.matvec_terms64(wq, ws, xq, xs, gs), 3, f"n {n} gs {gs} d {d}")


# ---------------------------------------------------------------- b + c. several pairs a wave; the epilogues, exact
def at_three_grids(gpu, epi, gs, segs, units_one_block=3, **kw):
    """The same launch at the default grid, in one block and in three: the grids and units a wave the case was built
    for, and every output bit equal across the three.  Returns {grid name: result}."""
    out = {}
    for which, over in GRIDS.items():
        res = gpu.q8_matvec_case(epi, gs, segs, **over, **kw)
        assert res["grid"] == expected_grid(res["n_pairs"], which), (which, res["grid"], res["n_pairs"])
        out[which] = res
    assert units_per_wave(out["default"]) == 1
    assert units_per_wave(out["one"]) == ceil_div(out["one"]["n_pairs"], 4) >= units_one_block
    for which in ("one", "three"):
        for a, b in zip(out["default"]["outs"], out[which]["outs"]):
            np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{epi}: default grid against {which}")
    return out


ROWS = [23, 24, 50]   # 23: the last pair's second row is clamped onto its first


@pytest.mark.parametrize("rows", ROWS)
def test_store_is_the_same_bits_at_every_grid(gpu, rows):
    n, gs = 288, 32
    rng = np.random.default_rng(rows)
    wq, ws = weights(rng, rows, n, gs)
    xq, xs = quantized_x(rng, n, gs)
    guard = np.full(rows + 3, 7.25, f32)   # (the floats behind the rows come back as they went in)
    out = at_three_grids(gpu, "store", gs, [(wq, ws)], xq=xq, xs=xs, outs=[guard])
    y = out["default"]["outs"][0]
    check_bound(y[:rows], ref_q8.matvec_terms64(wq, ws, xq, xs, gs), 3, f"store rows {rows}")
    np.testing.assert_array_equal(y[rows:], guard[rows:])
    # ... and as three segments whose borders fall inside a pair: the rows land in their own segment's output
    cut = [rows // 3 | 1, rows // 3 | 1, rows - 2 * (rows // 3 | 1)]
    at = np.cumsum([0] + cut)
    segs = [(wq[at[j]:at[j + 1]], ws[at[j]:at[j + 1]]) for j in range(3)]
    out3 = at_three_grids(gpu, "store", gs, segs, xq=xq, xs=xs)
    np.testing.assert_array_equal(bits(np.concatenate(out3["default"]["outs"])), bits(y[:rows]))


def test_store_across_both_loops_at_once(gpu):
    """n 4160 (two batches a row) and 23 rows in one block (three pairs a wave): the batch loop inside the unit loop"""
    n, gs, rows = 4160, 64, 23
    rng = np.random.default_rng(4160)
    wq, ws = weights(rng, rows, n, gs)
    xq, xs = quantized_x(rng, n, gs)
    runs_past_the_first_batch(rng, wq, xq)
    out = at_three_grids(gpu, "store", gs, [(wq, ws)], xq=xq, xs=xs)
    assert ceil_div(n, BATCH) == 2 and out["one"]["grid"] == 1 and units_per_wave(out["one"]) == 3
    check_bound(out["one"]["outs"][0], ref_q8.matvec_terms64(wq, ws, xq, xs, gs), 3, "n 4160, 23 rows, one block")


@pytest.mark.parametrize("rows", ROWS)
def test_resid_is_the_residual_plus_the_store_sums_at_every_grid(gpu, rows):
    """out == f32(resid + y) bit for bit, out of place and in place (out0 == resid, as the pass's Wo and W2 launches),
    x in f32 without a norm as those launches take it"""
    n, gs = 288, 32
    rng = np.random.default_rng(100 + rows)
    wq, ws = weights(rng, rows, n, gs)
    x, _ = float_x(rng, n)
    resid = (rng.standard_normal(rows) * 3).astype(f32)
    y = gpu.q8_matvec_case("store", gs, [(wq, ws)], x=x)["outs"][0]
    assert np.abs(y).min() > 0 and len(set(resid.tolist())) == rows   # (a residual from another pair shows)
    want = (resid + y).astype(f32)
    apart = at_three_grids(gpu, "resid", gs, [(wq, ws)], x=x, resid=resid)
    place = at_three_grids(gpu, "resid", gs, [(wq, ws)], x=x, in_place=True, outs=[resid])
    for which in GRIDS:
        np.testing.assert_array_equal(bits(apart[which]["outs"][0]), bits(want), err_msg=f"out of place, {which}")
        np.testing.assert_array_equal(bits(place[which]["outs"][0]), bits(want), err_msg=f"in place, {which}")


def test_swiglu_is_silu_of_one_sum_times_the_other_at_every_grid(gpu):
    """13 pairs of the interleaved W1 | W3 slot, the rmsnorm in the kernel: against the float64 value of
    sa / (1 + exp(-sa)) * sb on the store epilogue's sums of the two rows, 8 * 2^-24 relative (expf within about an ulp,
    plus four roundings)."""
    n, gs, pairs = 288, 32, 13
    rng = np.random.default_rng(13)
    wq, ws = weights(rng, 2 * pairs, n, gs)
    x, g = float_x(rng, n)
    y = gpu.q8_matvec_case("store", gs, [(wq, ws)], x=x, rms_w=g)["outs"][0].astype(np.float64)
    sa, sb = y[0::2], y[1::2]
    assert np.abs(sa).max() > 1 and np.abs(sa).max() < 40
    want = sa / (1.0 + np.exp(-sa)) * sb
    out = at_three_grids(gpu, "swiglu", gs, [(wq, ws)], units_one_block=4, x=x, rms_w=g, outs=[np.full(pairs + 2, 7.25, f32)])
    got = out["default"]["outs"][0]
    np.testing.assert_array_equal(got[pairs:], np.full(2, 7.25, f32))
    ratio = np.abs(got[:pairs] - want) / (8 * 2.0 ** -24 * np.abs(want))
    print(f"swiglu: worst error / bound {ratio.max():.3f}")
    assert np.all(ratio <= 1), f"pairs over 8 * 2^-24 relative: {np.flatnonzero(ratio > 1)}, worst ratio {ratio.max():.3g}"


ROPE_SHAPES = [(4, 2, 16), (6, 6, 48), (2, 1, 64)]   # (heads, kv heads, head size): GQA, the 288 shape, one wide head
SEQ_LEN = 5


@pytest.mark.parametrize("pos", [0, 1, SEQ_LEN - 1])
@pytest.mark.parametrize("n_heads,n_kv,hs", ROPE_SHAPES)
def test_rope_rotates_q_and_k_and_writes_the_head_major_cache_at_every_grid(gpu, n_heads, n_kv, hs, pos):
    """q and K equal sa * c - sb * s and sa * s + sb * c in f32 (two products and one add, each rounded: the kernels are
    built without contraction) with c, s of (pos, (row % head_size) / 2); V is the sums themselves; K and V land at
    [kv head][pos][i] and every other float of the caches keeps what it held."""
    dim, kvd = n_heads * hs, n_kv * hs
    n, gs = dim, 32
    rng = np.random.default_rng(dim * 7 + pos)
    segs = [weights(rng, r, n, gs) for r in (dim, kvd, kvd)]
    x, g = float_x(rng, n)
    table = rng.uniform(-1, 1, (pos + 1, hs // 2, 2)).astype(f32)   # every (position, pair) its own cos / sin
    ys = gpu.q8_matvec_case("store", gs, segs, x=x, rms_w=g)["outs"]
    assert all(np.abs(y).min() > 0 for y in ys)

    def rotated(y):
        a = y.reshape(-1, hs // 2, 2)
        sa, sb, c, s = a[:, :, 0], a[:, :, 1], table[pos, :, 0], table[pos, :, 1]
        o0 = ((sa * c).astype(f32) - (sb * s).astype(f32)).astype(f32)
        o1 = ((sa * s).astype(f32) + (sb * c).astype(f32)).astype(f32)
        return np.stack([o0, o1], axis=2).reshape(-1)

    fill = [np.full(dim, 7.25, f32)] + [(np.arange(n_kv * SEQ_LEN * hs) * 0.5 + 1000 * j).astype(f32) for j in (1, 2)]
    want = [rotated(ys[0])]
    for j, rows in ((1, rotated(ys[1])), (2, ys[2])):
        cache = fill[j].copy().reshape(n_kv, SEQ_LEN, hs)
        cache[:, pos, :] = rows.reshape(n_kv, hs)
        want.append(cache.reshape(-1))
    out = at_three_grids(gpu, "rope", gs, segs, x=x, rms_w=g, outs=fill, rope=table, pos=pos, head_size=hs, rope_segs=2,
                         seq_len=SEQ_LEN)
    for which in GRIDS:
        for name, a, b in zip("qkv", out[which]["outs"], want):
            np.testing.assert_array_equal(bits(a), bits(b), err_msg=f"{name}, {which} grid")


def scan(y):
    """the reference's scan (main.zig:715-726) on a row without NaNs: the lowest index of the largest value"""
    return int(np.argmax(y))


def fold(part_val, part_idx):
    """argmax_rule.h's merge over the per-block candidates: larger value wins, equal values take the lower index"""
    best_v, best_i = -np.inf, 0x7FFFFFFF
    for v, i in zip(part_val.tolist(), part_idx.tolist()):
        if v > best_v or (v == best_v and i < best_i):
            best_v, best_i = v, i
    return best_i


def check_argmax(res, y, what):
    rows, grid = y.size, res["grid"]
    np.testing.assert_array_equal(bits(res["outs"][0][:rows]), bits(y), err_msg=f"{what}: the logits are the store sums")
    assert fold(res["part_val"], res["part_idx"]) == scan(y), what
    # every block's candidate is the scan over the block's own rows: pair u belongs to block (u / 4) % grid
    block_of_row = (np.arange(rows) // 8) % grid
    for b in range(grid):
        mine = np.flatnonzero(block_of_row == b)
        assert res["part_idx"][b] == mine[scan(y[mine])], f"{what}: block {b}"
        assert bits(res["part_val"][b])[0] == bits(y[res["part_idx"][b]])[0], f"{what}: block {b}"


def rows_that_tie_at_the_top(wq, ws, x, g, dup):
    """rows `dup` become one and the same row whose sum is the largest of all: +-127 with the sign of the normalised
    x (the rmsnorm factor is positive) and scales above every other row's"""
    v = x * (g if g is not None else 1.0)
    wq[dup] = np.where(v >= 0, 127, -127).astype(np.int8)
    ws[dup] = f32(0.05)


@pytest.mark.parametrize("rows,dup", [(23, [22]), (24, [2, 3, 11, 20]), (50, [12, 13, 22, 37, 49]), (50, [47, 30, 31])])
def test_argmax_candidates_fold_to_the_reference_scan_at_every_grid(gpu, rows, dup):
    """The classifier's epilogue: the logits are the store sums, and the per-block candidates fold to the scan's index.
    Rows with EQUAL sums by construction (one row's values and scales at several places) sit in both rows of one pair,
    in other waves, in later units of the same wave and in other blocks: the lowest index wins at every grid."""
    n, gs = 288, 32
    rng = np.random.default_rng(rows * 3 + len(dup))
    wq, ws = weights(rng, rows, n, gs)
    x, g = float_x(rng, n)
    rows_that_tie_at_the_top(wq, ws, x, g, dup)
    y = gpu.q8_matvec_case("store", gs, [(wq, ws)], x=x, rms_w=g)["outs"][0]
    top = np.flatnonzero(y == y.max())
    assert top.tolist() == sorted(dup) and len(set(bits(y[dup]).tolist())) == 1, "the rows built to tie are the maxima, bit for bit"
    out = at_three_grids(gpu, "argmax", gs, [(wq, ws)], x=x, rms_w=g, outs=[np.full(rows + 1, 7.25, f32)])
    for which, res in out.items():
        assert res["outs"][0][rows] == f32(7.25)
        check_argmax(res, y, f"rows {rows}, ties {dup}, {which} grid")
        assert fold(res["part_val"], res["part_idx"]) == min(dup)


def test_argmax_at_a_classifier_sized_row_count(gpu):
    """20000 rows at n = 64, the default grid: more pairs than resident waves, so a wave takes at least two pairs and
    hands over the better of several candidates -- the one check here that rests on the device's occupancy."""
    rows, n, gs = 20000, 64, 32
    rng = np.random.default_rng(20000)
    wq, ws = weights(rng, rows, n, gs)
    x, g = float_x(rng, n)
    dup = [6000, 6001, 15001, 19999]
    rows_that_tie_at_the_top(wq, ws, x, g, dup)
    y = gpu.q8_matvec_case("store", gs, [(wq, ws)], x=x, rms_w=g)["outs"][0]
    assert np.flatnonzero(y == y.max()).tolist() == dup
    res = gpu.q8_matvec_case("argmax", gs, [(wq, ws)], x=x, rms_w=g)
    print(f"classifier-sized: grid {res['grid']}, {res['n_pairs']} pairs, units a wave {units_per_wave(res)}")
    assert units_per_wave(res) >= 2
    check_argmax(res, y, "20000 rows")
    assert fold(res["part_val"], res["part_idx"]) == 6000


# ---------------------------------------------------------------- d. the fused prologue, held tight
_identical = []   # (the fused run against q8_matmul on the reference's integers: counted, printed, not asserted)


@pytest.mark.parametrize("n,gs,norm", kc.PROLOGUE_CASES)
def test_fused_prologue_meets_the_tight_bound(gpu, n, gs, norm):
    """rmsnorm + group quantization in the kernel, on inputs whose sum of squares is exact in f32 in any order and whose
    quotients keep 2^-10 from every rounding boundary (tests/q8_kernel_cases.py; asserted in tests/test_ref_q8_cpu.py): the
    float64 reference's integers are then the only correct ones, the device's scales are at most 2 ulp off, and the
    product stays within (G + 8) * 2^-24 * sum |term| of the reference -- the (G + 3) of the product itself plus 5 for
    the scales."""
    x, rms_w, wq, ws = kc.prologue_case(n, gs, norm)
    xq, xs, margin, terms = kc.prologue_reference(n, gs, norm)
    assert not norm or margin >= kc.MARGIN
    res = gpu.q8_matvec_case("store", gs, [(wq, ws)], x=x, rms_w=rms_w)
    got = res["outs"][0]
    assert ceil_div(n, BATCH) == {288: 1, 4096: 1, 11008: 3}[n] and units_per_wave(res) == 1
    check_bound(got, terms, 8, f"prologue n {n} gs {gs} norm {norm}")
    same = bool(np.array_equal(bits(got), bits(gpu.q8_matmul(xq, xs, wq, ws, gs))))
    _identical.append(same)
    print(f"prologue: {sum(_identical)} of {len(_identical)} cases so far bit-identical to q8_matmul on the reference's integers")
    if not norm:   # the device's values are the input's own: its integers and scales are the rule's, bit for bit
        assert same


@pytest.mark.parametrize("n,gs", [(288, 32), (4096, 64), (11008, 32)])
def test_fused_quantization_of_the_rules_hard_groups_is_exact(gpu, n, gs):
    """test_gpu_q8.py's groups -- all zero, a denormal maximum, +-max at both ends, exact ties at +-0.5 ... +-126.5 -- through
    the kernel's own staging, without a norm: bit-identical to the product on the reference's integers and scales."""
    x = quantize_rows(n, gs)
    xq, xs = ref_q8.quantize_act(x, gs)
    assert xs.min() == 0 and np.abs(xq).max() == 127
    rng = np.random.default_rng(n + gs)
    wq, ws = weights(rng, kc.PROLOGUE_ROWS, n, gs)
    got = gpu.q8_matvec_case("store", gs, [(wq, ws)], x=x)["outs"][0]
    np.testing.assert_array_equal(bits(got), bits(gpu.q8_matmul(xq, xs, wq, ws, gs)))
    check_bound(got, ref_q8.matvec_terms64(wq, ws, xq, xs, gs), 3, f"hard groups n {n} gs {gs}")
