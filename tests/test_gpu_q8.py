"""Decode from int8 group-quantized weights (llama2.c version-2 checkpoints) on the GPU: the activation
rule and the weight rule bit for bit, the product against its derived bound, the whole pass against tests/ref_q8.py, the
loops against the stepped pass bit for bit, and the refusals.  tests/test_ref_q8_cpu.py checks on the CPU what these rely
on; tests/q8_cases.py holds the shared inputs and the two bars."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cases  # noqa: E402
import ref_q8  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------- 1. the activation rule, exact
def quantize_rows(n, gs):
    """n values whose groups cycle through: random, exact ties, all zero, a denormal maximum, +-max at both ends."""
    rng = np.random.default_rng(n * 131 + gs)
    x = rng.standard_normal(n).astype(f32) * f32(3.0)
    g = x.reshape(-1, gs)
    for i in range(g.shape[0]):
        kind = i % 5
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
            m = f32(np.abs(g[i]).max() * 1.5)
            g[i, 0], g[i, -1] = -m, m
    return g.reshape(-1)


@pytest.mark.parametrize("n,gs", [(32, 32), (288, 32), (768, 32), (768, 64), (4096, 32), (4096, 64), (11008, 32), (11008, 64)])
def test_quantize_matches_the_rule_bit_for_bit(gpu, n, gs):
    x = quantize_rows(n, gs)
    q_ref, s_ref = ref_q8.quantize_act(x, gs)
    if n // gs >= 5:
        assert s_ref.min() == 0 and np.any((s_ref > 0) & (s_ref < 1e-38)), "the rows hold a zero and a denormal group"
    q, s = gpu.q8_quantize(x, gs)
    np.testing.assert_array_equal(bits(s), bits(s_ref))
    np.testing.assert_array_equal(q, q_ref)


# ---------------------------------------------------------------- 2. the weight rule, exact
@pytest.mark.parametrize("name", ["64", "288"])
def test_weights_quantized_on_the_device_and_loaded_from_a_file_are_the_rule(gpu, ck, tmp_path, name):
    cfg, gs, blob, body = q8_cases.model(name)
    path = tmp_path / "model_q80.bin"
    ck.write_checkpoint_v2(path, cfg, body, True, gs)
    cfg2, shared2, gs2, body2 = ck.read_checkpoint_v2(path)
    assert (cfg2, shared2, gs2) == (cfg, True, gs)
    w32 = gpu.Weights(cfg, blob, True)
    wq = gpu.Weights.quantized(w32, gs)
    w32.close()   # the quantized object is independent of its source
    wf = gpu.Weights.from_q8(cfg2, body2, shared2, gs2)
    t = ck.carve(cfg, blob, True)
    for tensor in ck.V2_QUANTIZED:
        layers = 1 if tensor in ("token_embedding_table", "wcls") else cfg.n_layers
        for l in range(layers):
            src = t[tensor] if layers == 1 else t[tensor][l]
            q_ref, s_ref = ck.quantize_q80(src, gs)
            for w in (wq, wf):
                q, s = w.q8_read(tensor, l)
                np.testing.assert_array_equal(q, q_ref, err_msg=f"{tensor} layer {l}")
                np.testing.assert_array_equal(bits(s).reshape(-1), bits(s_ref), err_msg=f"{tensor} layer {l}")
    with pytest.raises(gpu.L2ZError) as e:
        wq.read(0, 4)
    assert e.value.code == gpu.ERR_INVALID
    wq.close(); wf.close()


# ---------------------------------------------------------------- 3. the product, derived bound
MATVEC_CASES = [(n, d, gs) for n, d in ((64, 7), (288, 288), (768, 288), (1408, 512), (4096, 130)) for gs in (32, 64) if n % gs == 0]


@pytest.mark.parametrize("n,d,gs", MATVEC_CASES)
@pytest.mark.parametrize("fill", ["random", "extreme"])
def test_matmul_meets_the_derived_bound(gpu, n, d, gs, fill):
    """Against the float64 value of sum_g f32(I) * ws * xs with the exact integer sums: two roundings a term and any order
    of the f32 sum stay within (G + 3) * 2^-24 * sum_g |term_g|, G = n / gs."""
    rng = np.random.default_rng(n * 7 + d * 3 + gs)
    if fill == "random":
        wq = rng.integers(-127, 128, (d, n)).astype(np.int8)
        xq = rng.integers(-127, 128, n).astype(np.int8)
    else:   # +-127 everywhere: the int32 range of a group (64 * 127 * 127), all one sign in the first rows
        wq = np.where(rng.integers(0, 2, (d, n)) > 0, 127, -127).astype(np.int8)
        xq = np.where(rng.integers(0, 2, n) > 0, 127, -127).astype(np.int8)
        wq[0] = xq
        if d > 1:
            wq[1] = -xq
    ws = (rng.random((d, n // gs)) * 0.02 + 1e-4).astype(f32)
    xs = (rng.random(n // gs) * 0.05 + 1e-4).astype(f32)
    got = gpu.q8_matmul(xq, xs, wq, ws, gs).astype(np.float64)
    terms = ref_q8.matvec_terms64(wq, ws, xq, xs, gs)
    ref = terms.sum(axis=1)
    bound = (n // gs + 3) * 2.0 ** -24 * np.abs(terms).sum(axis=1)
    err = np.abs(got - ref)
    print(f"n {n} d {d} gs {gs} {fill}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound), f"rows over the bound: {np.flatnonzero(err > bound)[:8]}"
    if fill == "extreme":
        assert abs(int(ref_q8.group_sums(wq[:1], xq, gs)[0, 0])) == gs * 127 * 127
    again = gpu.q8_matmul(xq, xs, wq, ws, gs)
    np.testing.assert_array_equal(bits(again), bits(got.astype(f32)))


# ---------------------------------------------------------------- 4. the whole pass
def run_device(gpu, name, w=None):
    cfg, gs, _, body = q8_cases.model(name)
    own = w is None
    if own:
        w = gpu.Weights.from_q8(cfg, body, True, gs)
    s = gpu.RunState(cfg)
    zs = []
    for pos, tok in enumerate(q8_cases.tokens(name)):
        s.transformer(int(tok), pos, w)
        zs.append(s.logits())
    L, S, kvd, P = cfg.n_layers, cfg.seq_len, cfg.kv_dim, q8_cases.N_POS
    k = np.stack([s.read("key_cache", l * S * kvd, P * kvd).reshape(P, kvd) for l in range(L)])
    v = np.stack([s.read("value_cache", l * S * kvd, P * kvd).reshape(P, kvd) for l in range(L)])
    s.close()
    if own:
        w.close()
    return np.stack(zs), k, v


@pytest.mark.parametrize("name", list(q8_cases.SHAPES))
def test_whole_pass_against_the_float64_reference(gpu, name):
    """Twelve positions: logits and every layer's K / V rows meet the project's parity bar, except at most ONE position,
    which stays under the loose bar (q8_cases.LOOSE): the device's summation order may put one activation on the other
    side of a rounding boundary.  (The two CPU modes need no exception on these inputs: tests/test_ref_q8_cpu.py.)"""
    z, k, v = run_device(gpu, name)
    ok, dev = q8_cases.check_positions(z, k, v, *q8_cases.reference(name, "f64"), exceptions=1)
    print(f"shape {name}: positions over the parity bar {list(np.flatnonzero(~ok))}, largest deviation {dev.max():.3e} of the scale")
    z2, k2, v2 = run_device(gpu, name)   # the same bits from run to run
    for a, b in ((z, z2), (k, k2), (v, v2)):
        np.testing.assert_array_equal(bits(a), bits(b))


def test_weights_quantized_on_the_device_run_the_same_pass(gpu):
    """l2z_weights_init_q8_from holds the file's values (test 2), so the pass on it gives the file's bits."""
    cfg, gs, blob, _ = q8_cases.model("288")
    w32 = gpu.Weights(cfg, blob, True)
    w = gpu.Weights.quantized(w32, gs)
    w32.close()
    for a, b in zip(run_device(gpu, "288", w), run_device(gpu, "288")):
        np.testing.assert_array_equal(bits(a), bits(b))
    w.close()


# ---------------------------------------------------------------- 5. the loops
PROMPT = [5, 9, 300, 41, 77]


def test_greedy_run_emits_the_ids_of_the_reference(gpu):
    """16 steps after a 5-token prompt on the checkpoint built for it (q8_cases.peaked_model; classifier not shared): the
    reference's top-2 margin is at least 10 x the loose bar, as a fraction of the logit scale, at every step -- no flipped
    activation can change an id --, and the loop emits the reference's ids."""
    ids_ref, margins, zs = q8_cases.peaked_reference()
    scale = np.abs(zs).max(axis=1)
    print(f"top-2 margins {np.min(margins / scale):.2f} .. {np.max(margins / scale):.2f} of the logit scale, needed {10 * q8_cases.LOOSE:.2f}")
    assert np.all(margins >= 10 * q8_cases.LOOSE * scale)
    assert 1 not in ids_ref and list(ids_ref[:5]) == q8_cases.GREEDY_PROMPT
    cfg, gs, body = q8_cases.peaked_model()
    w = gpu.Weights.from_q8(cfg, body, False, gs)
    s = gpu.RunState(cfg)
    s.greedy_begin(q8_cases.GREEDY_PROMPT)
    ids = s.greedy_run(w, q8_cases.GREEDY_STEPS)
    np.testing.assert_array_equal(ids, ids_ref)
    assert q8_cases.parity_ok(s.logits(), zs[-1]) or q8_cases.scaled_dev(s.logits(), zs[-1]) <= q8_cases.LOOSE
    s.close(); w.close()


@pytest.mark.parametrize("name", ["288", "tall"])
def test_greedy_run_is_the_stepped_loop_bit_for_bit(gpu, name):
    """("tall": the classifier's waves take several pairs each, so the loop's hand-over from several candidates a wave is
    held to s.argmax().)"""
    cfg, gs, _, body = q8_cases.model(name)
    w = gpu.Weights.from_q8(cfg, body, True, gs)
    runs = []
    for _ in range(2):
        s = gpu.RunState(cfg)
        s.greedy_begin(PROMPT)
        ids = s.greedy_run(w, 16)
        runs.append((ids, s.logits()))
        s.close()
    assert len(runs[0][0]) == 16 and list(runs[0][0][:5]) == PROMPT
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(bits(runs[0][1]), bits(runs[1][1]))
    # the stepped loop: l2z_transformer position by position, the prompt forced, else the argmax
    s = gpu.RunState(cfg)
    tok, ids = 1, []
    for pos in range(16):
        s.transformer(tok, pos, w)
        tok = PROMPT[pos] if pos < len(PROMPT) else s.argmax()
        ids.append(tok)
    np.testing.assert_array_equal(np.array(ids, np.int32), runs[0][0])
    np.testing.assert_array_equal(bits(s.logits()), bits(runs[0][1]))
    s.close(); w.close()


def test_sample_run_is_the_stepped_loop_plus_sample_batch_bit_for_bit(gpu):
    cfg, gs, _, body = q8_cases.model("288")
    w = gpu.Weights.from_q8(cfg, body, True, gs)
    coins = gpu.coin_stream(7, 16)
    runs = []
    for _ in range(2):
        s = gpu.RunState(cfg)
        ids = gpu.generate_sample(s, w, PROMPT, 16, 1.0, 0.9, coins)
        runs.append((ids, s.logits()))
        s.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(bits(runs[0][1]), bits(runs[1][1]))
    s = gpu.RunState(cfg)
    tok, ids, g = 1, [], 0
    for pos in range(16):
        s.transformer(tok, pos, w)
        if pos < len(PROMPT):
            tok = PROMPT[pos]
        else:
            tok = int(gpu.sample_batch([s], 1.0, 0.9, coins[g])[0])
            g += 1
        ids.append(tok)
        if tok == 1:
            break
    np.testing.assert_array_equal(np.array(ids, np.int32), runs[0][0])
    np.testing.assert_array_equal(bits(s.logits()), bits(runs[0][1]))
    s.close(); w.close()


def test_time_kind_and_profile_forward_take_q8_weights(gpu):
    cfg, gs, _, body = q8_cases.model("64")
    w = gpu.Weights.from_q8(cfg, body, True, gs)
    s = gpu.RunState(cfg)
    for kind in ("qkv", "attn", "wo", "ffn13", "ffn2", "cls", "argmax"):
        ms, n = s.time_kind(kind, 3, w, reps=2)
        assert ms > 0 and n == 2 * (1 if kind in ("cls", "argmax") else cfg.n_layers)
    prof = s.profile_forward(5, 0, w)
    assert prof["qkv"][1] == cfg.n_layers and prof["cls"][1] == 1 and prof["argmax"][1] == 1
    s.close(); w.close()


# ---------------------------------------------------------------- 6. refusals
def test_every_other_entry_point_refuses_q8_weights_and_changes_nothing(gpu):
    B = gpu
    cfg, gs, _, body = q8_cases.model("64")
    w = B.Weights.from_q8(cfg, body, True, gs)
    s, s2, twin = B.RunState(cfg), B.RunState(cfg), B.RunState(cfg)
    for r in (s, twin):
        r.greedy_begin(PROMPT)
        r.greedy_run(w, 7)
    s2.transformer(3, 0, w)
    S, kvd = cfg.seq_len, cfg.kv_dim
    before = (s.logits(), s.read("key_cache", (S + 4) * kvd, kvd), s.read("value_cache", 2 * kvd, kvd))
    toks = [7, 8, 9]
    calls = {
        "l2z_prefill": lambda: s.prefill(toks, 7, w),
        "l2z_score": lambda: s.score(toks, 7, w),
        "l2z_transformer_batch": lambda: B.transformer_batch([s, s2], [7, 8], [7, 1], w),
        "l2z_batch_time": lambda: B.batch_time([s, s2], [7, 8], [7, 1], w, 1),
        "l2z_verify": lambda: s.verify(toks, 7, w),
        "l2z_verify_time": lambda: s.verify_time(toks, 7, w, 1),
        "l2z_verify_sample": lambda: s.verify_sample(toks, 7, w, 1.0, 0.9, [0.1, 0.2, 0.3]),
        "l2z_verify_tree": lambda: s.verify_tree(toks, [-1, 0, 0], 7, w),
        "l2z_verify_batch": lambda: B.verify_batch([s, s2], [toks, toks], [7, 1], w),
        "l2z_verify_wide": lambda: B.verify_wide([s, s2], [toks, toks], [7, 1], w),
        "l2z_prefill_batch": lambda: B.prefill_batch([s, s2], [toks, toks], [7, 1], w),
        "l2z_transformer_wide": lambda: B.transformer_wide([s, s2], [7, 8], [7, 1], w),
        "l2z_wide_run": lambda: B.wide_run([s, s2], [7, 8], [7, 1], w, 2),
        "l2z_step_mixed": lambda: B.step_mixed([s, s2], [toks, [8]], [7, 1], w),
        "l2z_emu_transformer": lambda: B.emu_transformer([s], [w], 7, 7),
        "l2z_emu_prefill": lambda: B.emu_prefill([s, s2], [w, w], toks, 7),
    }
    for name, call in calls.items():
        with pytest.raises(B.L2ZError) as e:
            call()
        assert e.value.code == B.ERR_INVALID, f"{name}: {e.value}"
        assert "l2z_greedy_run" in str(e.value), f"{name}: the message names the supported calls: {e.value}"
    after = (s.logits(), s.read("key_cache", (S + 4) * kvd, kvd), s.read("value_cache", 2 * kvd, kvd))
    for a, b in zip(before, after):
        np.testing.assert_array_equal(bits(a), bits(b))
    # ... and the next position: the loop goes on exactly as its undisturbed twin's
    np.testing.assert_array_equal(s.greedy_run(w, 5), twin.greedy_run(w, 5))
    np.testing.assert_array_equal(bits(s.logits()), bits(twin.logits()))
    # a paged runstate is refused as with f32 weights; a runstate of a shard group is refused
    pool = B.KvPool(cfg, 4)
    sp = B.RunState(cfg, pool=pool)
    with pytest.raises(B.L2ZError) as e:
        sp.transformer(3, 0, w)
    assert e.value.code == B.ERR_INVALID
    sp.close(); pool.close()
    comm = B.Comm(0, 2, None, 0, emulated=True)
    ss = B.RunState(cfg, comm=comm)
    with pytest.raises(B.L2ZError) as e:
        ss.transformer(3, 0, w)
    assert e.value.code == B.ERR_INVALID
    ss.close(); comm.close()
    for r in (s, s2, twin):
        r.close()
    w.close()


def test_the_constructors_refuse_what_the_format_does_not_hold(gpu, ck):
    B = gpu
    cfg, gs, blob, body = q8_cases.model("64")

    def refused(fn):
        with pytest.raises(B.L2ZError) as e:
            fn()
        assert e.value.code == B.ERR_INVALID, str(e.value)

    refused(lambda: B.Weights.from_q8(cfg, body, True, 16))                 # a group size the format does not have
    cfg288, _, blob288, body288 = q8_cases.model("288")
    refused(lambda: B.Weights.from_q8(cfg288, body288, True, 64))           # dim 288 is no multiple of 64
    refused(lambda: B.Weights.from_q8(cfg, body[:-1], True, gs))            # a truncated body
    refused(lambda: B.Weights.from_q8(cfg, body, False, gs))                # ... as is a shared file read as unshared
    comm = B.Comm(0, 2, None, 0, emulated=True)
    refused(lambda: B.Weights.from_q8(cfg, body, True, gs, comm=comm))      # a comm
    w_shard = B.Weights(cfg, blob, True, comm=comm)
    refused(lambda: B.Weights.quantized(w_shard, gs))                       # a sharded source
    w_shard.close(); comm.close()
    w32 = B.Weights(cfg, blob, True)
    refused(lambda: B.Weights.quantized(w32, 16))
    w288 = B.Weights(cfg288, blob288, True)
    refused(lambda: B.Weights.quantized(w288, 64))
    w288.close()
    wq = B.Weights.quantized(w32, gs)
    refused(lambda: B.Weights.quantized(wq, gs))                            # a quantized source
    wq.close(); w32.close()
