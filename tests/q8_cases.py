"""The inputs the int8 group-quantized tests share (tests/test_ref_q8_cpu.py checks on the CPU what the GPU tests rely
on): the shapes, one seeded checkpoint a shape, the twelve tokens fed at positions 0 .. 11, the greedy prompt, and the two
bars the whole-pass comparison uses.

Shapes are (dim, hidden_dim, layers, heads, kv heads, vocab, seq_len, group size): the smallest at which the kernel can
still go wrong -- 9 groups a row, odd pair counts, GQA, a hidden size that is no power of two.
"""
import functools

import numpy as np

SHAPES = {
    "64": (64, 192, 2, 4, 2, 512, 32, 32),
    "288": (288, 768, 3, 6, 6, 1024, 32, 32),
    "512": (512, 1408, 4, 8, 8, 512, 24, 64),
    # both loops of the kernel in the real pass: W2 rows of 4224 columns are 1.03 batches of 4096, and the classifier's
    # 10000 pairs are more than the resident waves, so a wave takes several pairs and hands over several candidates
    "tall": (64, 4224, 1, 2, 1, 20000, 16, 64),
}
SEEDS = {"64": 59, "288": 24, "512": 121, "tall": 799}   # (picked for the largest distance of any activation quotient to a rounding boundary; "tall": 6.6e-5 of a step, the best of seeds 0 .. 999)
N_POS = 12

# The project's parity bar, elementwise: |got - ref| <= 5e-5 + 5e-5 |ref|.  And the LOOSE bar of the one position in
# twelve where the device's summation order may put an activation on the other side of a rounding boundary: there the
# largest |got - ref| of the position's logits, and of its K and of its V rows of every layer, each divided by the largest
# |ref| of the same (the logit scale, the rows' scale), stays under LOOSE.  LOOSE is 4 x the largest such deviation between
# the two modes of tests/ref_q8.py over a sweep of 756 positions of these shapes (21 seeded checkpoints a shape, positions
# where an element flipped included; scripts/q8_loose_bar.py): a flip moves one term of one sum, and a
# second arithmetic order may flip a different, larger term.
PARITY_RTOL = PARITY_ATOL = 5e-5
LOOSE_MEASURED = 0.0275   # largest deviation of the sweep, as a fraction of the scale
LOOSE = 4 * LOOSE_MEASURED


def config(ck, name):
    return ck.Config(*SHAPES[name][:7]), SHAPES[name][7]


@functools.lru_cache(maxsize=None)
def _model(name, seed):
    import __graft_entry__ as ge
    ck = ge.load_package().checkpoint
    cfg, gs = config(ck, name)
    blob = ck.synth_blob(cfg, True, seed)
    return cfg, gs, blob, ck.v2_body_from_f32(cfg, blob, True, gs)


def model(name, seed=None):
    """(cfg, gs, the f32 blob, the version-2 body quantized from it); shared classifier."""
    return _model(name, SEEDS[name] if seed is None else seed)


def tokens(name, seed=None):
    cfg = model(name, seed)[0]
    rng = np.random.default_rng(1000 + (SEEDS[name] if seed is None else seed))
    return rng.integers(2, cfg.vocab_size, N_POS).astype(np.int32)


def parity_ok(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.all(np.abs(got - ref) <= PARITY_ATOL + PARITY_RTOL * np.abs(ref)))


def scaled_dev(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def position_report(z_got, k_got, v_got, z_ref, k_ref, v_ref):
    """Per position (logits [P, V]; K / V rows [L, P, kvd]): whether everything of it meets the parity bar, and its
    largest deviation as a fraction of the scale (logits, K rows, V rows each against their own)."""
    P = z_ref.shape[0]
    ok = np.array([parity_ok(z_got[p], z_ref[p]) and parity_ok(k_got[:, p], k_ref[:, p]) and parity_ok(v_got[:, p], v_ref[:, p])
                   for p in range(P)])
    dev = np.array([max(scaled_dev(z_got[p], z_ref[p]), scaled_dev(k_got[:, p], k_ref[:, p]), scaled_dev(v_got[:, p], v_ref[:, p]))
                    for p in range(P)])
    return ok, dev


def check_positions(z_got, k_got, v_got, z_ref, k_ref, v_ref, exceptions):
    """The whole-pass rule: every position meets the parity bar, except at most `exceptions` of them, which stay under
    LOOSE.  Returns the report for printing."""
    ok, dev = position_report(z_got, k_got, v_got, z_ref, k_ref, v_ref)
    bad = [int(p) for p in np.flatnonzero(~ok)]
    assert len(bad) <= exceptions, f"positions over the parity bar: {bad}, deviations {dev[bad]}"
    assert all(dev[p] <= LOOSE for p in bad), f"position {bad} over the loose bar {LOOSE}: {dev[bad]}"
    return ok, dev


@functools.lru_cache(maxsize=None)
def reference(name, mode="f64"):
    """(logits [12, V], K rows [L, 12, kvd], V rows) of the shape's checkpoint and tokens, computed once"""
    import __graft_entry__ as ge
    import ref_q8
    ck = ge.load_package().checkpoint
    cfg, gs, _, body = model(name)
    z, m = ref_q8.run_positions(ck, cfg, body, True, gs, tokens(name), mode)
    return z, m.kc[:, :N_POS].copy(), m.vc[:, :N_POS].copy()


# ---- the greedy loop's checkpoint: top-2 margins of at least 10 x LOOSE of the logit scale at every step ----
# No seeded random checkpoint has such margins (LOOSE is 11 % of the logit scale: every other logit would have to lie below
# zero), so this one is built for it, on the "512" shape (vocab = dim = 512), classifier not shared: token t's embedding is
# the unit vector e_t plus a little noise, the classifier's row j is +1 at every t with NEXT[t] == j and -0.4 elsewhere,
# the layers' output matrices are scaled down so that the residual stream stays near e_t.  The logits of token t are then
# about +22.6 at NEXT[t] and -9 everywhere else: greedy decoding walks t -> NEXT[t], never through BOS.
PEAKED_SHAPE, PEAKED_GS = (512, 1408, 4, 8, 8, 512, 24), 64
NEXT = 2 + (np.arange(512) * 37 + 11) % 510
GREEDY_PROMPT = [5, 9, 300, 41, 77]
GREEDY_STEPS = 16


@functools.lru_cache(maxsize=None)
def peaked_model():
    """(cfg, gs, version-2 body) of the greedy loop's checkpoint"""
    import __graft_entry__ as ge
    ck = ge.load_package().checkpoint
    cfg = ck.Config(*PEAKED_SHAPE)
    blob = ck.synth_blob(cfg, False, 77).copy()
    t = ck.carve(cfg, blob, False)
    rng = np.random.default_rng(77)
    t["token_embedding_table"][:] = np.eye(512, dtype=np.float32) + 0.004 * rng.standard_normal((512, 512)).astype(np.float32)
    t["wo"][:] *= np.float32(0.004)
    t["w2"][:] *= np.float32(0.004)
    t["wcls"][:] = np.float32(-0.4)
    t["wcls"][NEXT, np.arange(512)] = np.float32(1.0)
    return cfg, PEAKED_GS, ck.v2_body_from_f32(cfg, blob, False, PEAKED_GS)


@functools.lru_cache(maxsize=None)
def peaked_reference():
    """(ids, top-2 margins, logits) of GREEDY_STEPS steps after GREEDY_PROMPT, float64 mode"""
    import __graft_entry__ as ge
    import ref_q8
    cfg, gs, body = peaked_model()
    return ref_q8.greedy(ge.load_package().checkpoint, cfg, body, False, gs, GREEDY_PROMPT, GREEDY_STEPS, "f64")
