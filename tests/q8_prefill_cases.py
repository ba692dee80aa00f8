"""The inputs the tests of the batched prompt pass on int8 group-quantized weights share (DESIGN.md 4.24;
tests/test_q8_prefill_cpu.py checks on the CPU what tests/test_gpu_q8_prefill.py relies on): q8_cases' checkpoints (same
shapes, same seeds) with one token run a shape, the references of those runs, and the inputs of the row launch's tests.

Token runs.  "64" and "512" take longer runs than the decode tests' twelve positions -- default_rng(1000 + seed).integers(2,
V, n) with n = 32 and 24, whose first twelve are q8_cases.tokens -- so that a chunk spans two (three) token tiles of 16;
"288" and "tall" keep the twelve (the 32-token draw of "288" flips an activation between the two CPU modes at position
14 and every later position leaves the parity bar, so it is not used).  On every chosen run the two modes of tests/ref_q8.py
agree at the parity bar at EVERY position (test_q8_prefill_cpu.py), so an exception on the device is the device's
summation order alone.
"""
import functools

import numpy as np

import q8_cases

f32 = np.float32
RUN_LENGTH = {"64": 32, "288": 12, "512": 24, "tall": 12}


def tokens(name):
    cfg = q8_cases.model(name)[0]
    rng = np.random.default_rng(1000 + q8_cases.SEEDS[name])
    return rng.integers(2, cfg.vocab_size, RUN_LENGTH[name]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(name, mode="f64"):
    """(logits [P, V], K rows [L, P, kvd], V rows, the smallest distance of an activation quotient to a rounding boundary)
    of the shape's checkpoint on its token run, computed once; read-only."""
    import __graft_entry__ as ge
    import ref_q8
    ck = ge.load_package().checkpoint
    cfg, gs, _, body = q8_cases.model(name)
    toks = tokens(name)
    z, m = ref_q8.run_positions(ck, cfg, body, True, gs, toks, mode)
    out = (z, m.kc[:, :len(toks)].copy(), m.vc[:, :len(toks)].copy())
    for a in out:
        a.setflags(write=False)
    return out + (min(m.margins),)


def report(z_by_pos, k_got, v_got, z_ref, k_ref, v_ref):
    """Per position of K / V rows [L, P, kvd] -- with the logits of the positions z_by_pos {p: [V]} has --: whether it meets
    the parity bar, and its largest deviation as a fraction of the scale (q8_cases.position_report's measures)."""
    P = k_ref.shape[1]
    ok, dev = np.ones(P, bool), np.zeros(P)
    for p in range(P):
        pairs = [(k_got[:, p], k_ref[:, p]), (v_got[:, p], v_ref[:, p])]
        if p in z_by_pos:
            pairs.append((z_by_pos[p], z_ref[p]))
        ok[p] = all(q8_cases.parity_ok(g, r) for g, r in pairs)
        dev[p] = max(q8_cases.scaled_dev(g, r) for g, r in pairs)
    return ok, dev


def check_rule(z_by_pos, k_got, v_got, ref):
    """The whole-pass rule of the batched pass, q8_cases' bars unchanged: every position before the first one over the
    parity bar meets it (by definition of first), and every position from there on stays under q8_cases.LOOSE -- a flipped
    activation reaches all later positions through the cache.  Returns (flipped, ok, dev)."""
    ok, dev = report(z_by_pos, k_got, v_got, *ref[:3])
    bad = np.flatnonzero(~ok)
    if bad.size:
        first = int(bad[0])
        assert np.all(dev[first:] <= q8_cases.LOOSE), f"positions from {first} on over the loose bar {q8_cases.LOOSE}: {dev[first:]}"
    return bool(bad.size), ok, dev


# ---- the row launch's inputs ----
def hard_rows(m, n, gs):
    """[m, n]: every row's groups cycle through random, exact ties, all zero, a denormal maximum, +-max at both ends
    (tests/test_gpu_q8.py's quantize_rows, a row its own draw and the cycle shifted by the row)."""
    out = np.empty((m, n), f32)
    for r in range(m):
        rng = np.random.default_rng(n * 131 + gs + 7919 * r)
        x = rng.standard_normal(n).astype(f32) * f32(3.0)
        g = x.reshape(-1, gs)
        for i in range(g.shape[0]):
            kind = (i + r) % 5
            if kind == 1:    # max = 127 * 2^-3: the scale is 2^-3 exactly, and these quotients are exact ties
                s = f32(0.125)
                g[i] = rng.integers(-100, 100, gs).astype(f32) * s
                g[i, :8] = np.array([0.5, -0.5, 1.5, -1.5, 126.5, -126.5, 2.5, -2.5], f32) * s
                g[i, 9] = f32(127.0) * s
            elif kind == 2:
                g[i] = 0
            elif kind == 3:  # a denormal maximum (the scale is a smaller denormal, still above 0)
                g[i] = (rng.integers(-700000, 700000, gs).astype(np.float64) * 2.0 ** -149).astype(f32)
                g[i, 5] = f32(713000 * 2.0 ** -149)
            elif kind == 4:
                mx = f32(np.abs(g[i]).max() * 1.5)
                g[i, 0], g[i, -1] = -mx, mx
        out[r] = g.reshape(-1)
    return out


NORM_CASES = [(n, gs) for n in (288, 4096, 11008) for gs in (32, 64) if n % gs == 0]


def norm_rows(m, n, gs):
    """([m, n] rows, rms_w [n]) built like tests/q8_kernel_cases.py's prologue inputs: row 0 is that case's x -- integers
    times 2^-3, an exact sum of squares in any order, with the weight every quotient at least 2^-10 from a rounding
    boundary --, row r is it with the sign (-1)^r: the same sum of squares, the same distances."""
    import q8_kernel_cases
    x, rms_w, _, _ = q8_kernel_cases.prologue_case(n, gs, True)
    sign = np.where(np.arange(m) % 2 == 0, f32(1), f32(-1))
    return (sign[:, None] * x[None, :]).astype(f32), rms_w


def norm_reference(x, rms_w, gs):
    """The row launch's arithmetic in numpy f32, statement by statement: the sum of squares (exact on these inputs in any
    order), / n, + 1e-5, 1 / sqrt -- each one correctly rounded f32 operation --, (v * f) * g, then the activation rule.
    Returns (q [m, n], s [m, n // gs], the smallest distance of a quotient to a rounding boundary)."""
    import ref_q8
    m, n = x.shape
    q, s, margins = np.empty((m, n), np.int8), np.empty((m, n // gs), f32), []
    for r in range(m):
        exact = float(np.sum(x[r].astype(np.float64) ** 2))
        assert exact * 64 < 2 ** 24 and f32(exact) == exact
        f = f32(exact) / f32(n)
        f = f32(f + f32(1e-5))
        f = f32(f32(1.0) / np.sqrt(f, dtype=f32))
        v = ((x[r] * f).astype(f32) * rms_w).astype(f32)
        q[r], s[r] = ref_q8.quantize_act(v, gs, margins)
    return q, s, min(margins)
