"""The int8 KV cache of the wide q8 step (l2z_runstate_init_kv8, l2z_kv8_attention) on the GPU: 1. the
attention kernel against float64; 2. the written rows, and the fork's, bit for bit against the rule; 3. row independence;
4. the step against the float64 reference with int8 rows (tests/kv8_cases.py); 5. depth through the step.  The refusals are
tests/test_kv8_abi.py's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_cases  # noqa: E402
import q8_batch_cases as bc  # noqa: E402
import q8_cases  # noqa: E402
import ref_q8  # noqa: E402
from test_gpu_q8_batch import caches, fresh, same, weights  # noqa: E402,F401

pytestmark = pytest.mark.gpu
f32 = np.float32
S_KERNEL = 160   # no multiple of 64: the last segment is partial


def fresh8(gpu, cfg, w, history):
    """a kv8 runstate that holds `history`: the prompt pass on an f32 runstate, then the fork that quantizes its rows"""
    s = gpu.RunState(cfg, kv8=True)
    if len(history):
        src = fresh(gpu, cfg, w, history)
        gpu.runstate_fork(s, src, len(history))
        s.synchronize()
        src.close()
    return s


def dequant(q, s, hs):
    return q.astype(f32) * np.repeat(s, hs, axis=-1)


def raw(s, cfg):
    """every byte and scale of a kv8 runstate: [which][layer] -> (int8 [S, kvd], f32 [S, kv heads])"""
    return [[s.read_kv8(which, l, 0, cfg.seq_len) for l in range(cfg.n_layers)] for which in "kv"]


def same_raw(a, b, what, but=None):
    for wa, wb in zip(a, b):
        for (qa, sa), (qb, sb) in zip(wa, wb):
            keep = np.ones(len(qa), bool) if but is None else ~but
            np.testing.assert_array_equal(qa[keep], qb[keep], err_msg=what)
            same(sa[keep], sb[keep], what)


# ---------------------------------------------------------------- 1. the kernel against float64
def kernel_inputs(H, KVH, hs, pos, fill):
    rng, n, S = np.random.default_rng(H * 1000 + hs + len(fill)), len(pos), S_KERNEL
    q = rng.standard_normal((n, H * hs)).astype(f32)
    if fill == "random":   # scales over four decades: scores of up to a few units, so a few keys dominate
        k8, v8 = (rng.integers(-127, 128, (n, KVH, S, hs)).astype(np.int8) for _ in range(2))
        ks, vs = ((10.0 ** rng.uniform(-5, -1, (n, KVH, S))).astype(f32) for _ in range(2))
    else:   # the bytes at their ends, zero rows with scale 0, and one key 60 above the rest for every head
        sgn = np.where(rng.random((n, KVH, hs)) < 0.5, -1, 1)
        q = (np.abs(q).reshape(n, KVH, H // KVH, hs) * sgn[:, :, None, :]).reshape(n, H * hs).astype(f32)
        k8, v8 = (rng.choice(np.array([-128, -127, 127], np.int8), (n, KVH, S, hs)) for _ in range(2))
        mass = np.abs(q).reshape(n, KVH, H // KVH, hs).sum(axis=3).min(axis=2)   # the least sum |q| of a kv head's heads
        top = (80.0 * np.sqrt(hs) / (127.0 * mass)).astype(f32)
        ks = np.repeat((top / 100)[:, :, None], S, axis=2).astype(f32)
        vs = np.full((n, KVH, S), 0.01, f32)
        k8[:, :, 2::5], ks[:, :, 2::5] = 0, 0.0
        v8[:, :, 3::7], vs[:, :, 3::7] = 0, 0.0
        for i, p in enumerate(pos):
            k8[i, :, p // 2], ks[i, :, p // 2] = 127 * sgn[i], top[i]
    for i, p in enumerate(pos):   # rows beyond a row's position must not be read
        ks[i, :, p + 1:], vs[i, :, p + 1:] = np.nan, np.nan
    return q, k8, ks, v8, vs


def attention64(q, pos, k8, ks, v8, vs, H):
    n, KVH, _, hs = k8.shape
    out, gap = np.zeros((n, H * hs)), np.inf
    for i in range(n):
        T = pos[i] + 1
        for h in range(H):
            g = h // (H // KVH)
            K, V = (a[i, g, :T].astype(np.float64) * b[i, g, :T, None].astype(np.float64) for a, b in ((k8, ks), (v8, vs)))
            s = K @ q[i, h * hs:(h + 1) * hs].astype(np.float64) / np.sqrt(hs)
            e = np.exp(s - s.max())
            out[i, h * hs:(h + 1) * hs] = (e / e.sum()) @ V
            if T > 1:
                gap = min(gap, np.sort(s)[-1] - np.sort(s)[-2])
    return out, gap


@pytest.mark.parametrize("fill", ["random", "adversarial"])
@pytest.mark.parametrize("pos", [(0, 1, 63), (64, 65, 127), (159, 0, 64)])
@pytest.mark.parametrize("H,KVH,hs", [(4, 2, 16), (6, 6, 48), (6, 2, 32), (8, 1, 64), (2, 2, 128), (1, 1, 256), (2, 1, 4)])
def test_the_attention_meets_the_parity_bar_against_float64(gpu, H, KVH, hs, pos, fill):
    q, k8, ks, v8, vs = kernel_inputs(H, KVH, hs, pos, fill)
    want, gap = attention64(q, pos, k8, ks, v8, vs, H)
    assert fill == "random" or gap >= 60.0, f"the input's dominant key stands {gap} above the rest"
    got = gpu.kv8_attention(q, pos, k8, ks, v8, vs, H)
    err = np.abs(got.astype(np.float64) - want)
    print(f"heads {H}/{KVH} head_size {hs} pos {pos} {fill}: largest |got - ref| {err.max():.3e}, of the bar "
          f"{(err / (q8_cases.PARITY_ATOL + q8_cases.PARITY_RTOL * np.abs(want))).max():.3f}")
    assert np.all(np.isfinite(got)) and np.all(err <= q8_cases.PARITY_ATOL + q8_cases.PARITY_RTOL * np.abs(want))


# ---------------------------------------------------------------- 2. the written rows, bit for bit
@pytest.mark.parametrize("name", bc.EXACT_SHAPES)
def test_a_step_writes_the_rule_s_bytes_and_scales_and_no_other_row(gpu, weights, name):
    cfg, w, n = bc.model(name)[0], weights(name), 17
    S, kvd, hs = cfg.seq_len, cfg.kv_dim, cfg.head_size
    toks = np.resize(bc.tokens(name), n)
    pos = np.array([i * (S - 1) // (n - 1) for i in range(n)], np.int32)
    states, twins = ([gpu.RunState(cfg, kv8=k) for _ in range(n)] for k in (True, False))
    before = raw(states[3], cfg)
    gpu.transformer_wide_q8(states, toks, pos, w, want_next=False)
    gpu.transformer_wide_q8(twins, toks, pos, w, want_next=False)
    for i, (s, t) in enumerate(zip(states, twins)):
        p = int(pos[i])
        for which, name_f32 in (("k", "key_cache"), ("v", "value_cache")):
            q_want, s_want = ref_q8.quantize_act(t.read(name_f32, p * kvd, kvd), hs)
            q_got, s_got = s.read_kv8(which, 0, p, 1)
            np.testing.assert_array_equal(q_got[0], q_want, err_msg=f"{which} bytes of row {i}")
            same(s_got[0], s_want, f"{which} scales of row {i}")
            assert np.abs(q_want).max() == 127
            same(s.read(name_f32, p * kvd, kvd), dequant(q_want, s_want, hs), f"the dequantized {which} row of row {i}")
            assert all(np.abs(s.read_kv8(which, l, p, 1)[0]).max() == 127 for l in range(cfg.n_layers))
    same_raw(before, raw(states[3], cfg), "rows the call does not name", but=np.arange(S) == pos[3])
    for s in states + twins:
        s.close()


@pytest.mark.parametrize("name", ["kv24", "wide80"])
def test_a_fork_quantizes_f32_rows_and_copies_int8_ones(gpu, weights, name):
    cfg, w, toks, n_pos = bc.model(name)[0], weights(name), bc.tokens(name), 70
    S, kvd, hs = cfg.seq_len, cfg.kv_dim, cfg.head_size
    src = fresh(gpu, cfg, w, toks[:n_pos])
    dst, dst2 = gpu.RunState(cfg, kv8=True), gpu.RunState(cfg, kv8=True)
    gpu.transformer_wide_q8([dst, dst2], toks[:2], [100, 101], w, want_next=False)   # rows beyond the fork, to be left alone
    before = raw(dst, cfg)
    gpu.runstate_fork(dst, src, n_pos)
    same(dst.logits(), src.logits(), "the fork's logits")
    K, V = caches(src, cfg)
    for rows, got in zip((K, V), raw(dst, cfg)):
        for l, (q_got, s_got) in enumerate(got):
            q_want, s_want = ref_q8.quantize_act(rows[l, :n_pos], hs)
            np.testing.assert_array_equal(q_got[:n_pos].reshape(-1), q_want, err_msg=f"layer {l}")
            same(s_got[:n_pos].reshape(-1), s_want, f"layer {l}")
    same_raw(before, raw(dst, cfg), "rows from n_pos on", but=np.arange(S) < n_pos)
    gpu.runstate_fork(dst2, dst, n_pos)
    same_raw(raw(dst, cfg), raw(dst2, cfg), "kv8 from kv8", but=np.arange(S) >= n_pos)
    assert np.abs(dst2.read_kv8("k", 0, 101, 1)[0]).max() == 127
    for s in (src, dst, dst2):
        s.close()


# ---------------------------------------------------------------- 3. row independence, bit for bit
def test_a_sequence_s_step_does_not_depend_on_the_other_rows(gpu, weights):
    name = "64"   # kv_mul 2
    cfg, w, toks = bc.model(name)[0], weights(name), bc.tokens(name)
    S, V, n, slot = cfg.seq_len, cfg.vocab_size, 17, 9
    rng = np.random.default_rng(7)

    def run(o_tok, o_depth):
        depth = [5 if i == slot else int(o_depth[i]) for i in range(n)]
        states = [fresh8(gpu, cfg, w, toks[:5] if i == slot else toks[7:7 + depth[i]]) for i in range(n)]
        bystander = fresh8(gpu, cfg, w, toks[:4])
        before, z_by = [raw(s, cfg) for s in states], bystander.logits()
        gpu.transformer_wide_q8(states, [int(toks[5]) if i == slot else int(o_tok[i]) for i in range(n)], depth, w, want_next=False)
        for i, s in enumerate(states):
            same_raw(before[i], raw(s, cfg), f"cache rows the call does not name, runstate {i}", but=np.arange(S) == depth[i])
        same(bystander.logits(), z_by, "a runstate the call does not name")
        out = (states[slot].logits(),) + caches(states[slot], cfg)
        for s in states + [bystander]:
            s.close()
        return out

    o_tok, o_depth = rng.integers(2, V, n), rng.integers(0, min(S - 8, 20), n)
    first = run(o_tok, o_depth)
    assert np.abs(first[0]).max() > 0 and np.abs(first[1][:, 5]).max() > 0
    for what, got in {"other tokens": run(rng.integers(2, V, n), o_depth), "other depths": run(o_tok, (o_depth + 3) % min(S - 8, 20))}.items():
        for a, b in zip(first, got):
            same(a, b, what)


# ---------------------------------------------------------------- 4. the step against the float64 reference
@pytest.mark.parametrize("n", [17, 128])
@pytest.mark.parametrize("name", kv8_cases.SHAPES)
def test_the_step_meets_the_float64_reference_with_int8_rows(gpu, name, n):
    """Sequence j is stepped to position j mod 12 of the shape's reference run, every position through the step itself (the
    rows a prompt pass leaves are the f32 attention's, another history); the positions under the q8 family's rule."""
    cfg, gs, _, body = kv8_cases.model(name)
    w, toks, P = gpu.Weights.from_q8(cfg, body, True, gs), kv8_cases.tokens(name), q8_cases.N_POS
    states = [gpu.RunState(cfg, kv8=True) for _ in range(n)]
    for r in range(P):
        live = [s for j, s in enumerate(states) if j % P >= r]
        gpu.transformer_wide_q8(live, [int(toks[r])] * len(live), [r] * len(live), w, want_next=False)
    z = np.stack([states[p].logits() for p in range(P)])
    k, v = (np.stack([c[:, p] for p, c in enumerate(kv)], axis=1) for kv in zip(*[caches(states[p], cfg) for p in range(P)]))
    for j in range(P, n):
        same(states[j].logits(), z[j % P], f"row {j}")
    for s in states + [w]:
        s.close()
    ok, dev = q8_cases.check_positions(z, k, v, *kv8_cases.reference(name), 1)
    print(f"kv8, shape {name}, n {n}: positions over the parity bar {list(np.flatnonzero(~ok))}, largest deviation {dev.max():.3e} of the scale")


# ---------------------------------------------------------------- 5. depth through the step
def test_a_deep_sequence_crosses_three_segments_on_the_reference(gpu, ck, weights):
    """One sequence forked at 70 positions, stepped beside 16 shallow ones to position 130.  The reference starts from the
    SAME 70 rows (the f32 runstate's, through the rule: the fork's bytes, test 2) and is fed the same tokens; every step's
    logits under the family's rule: the parity bar, at most one step in twelve over it, and those under LOOSE."""
    name, n_pos, last = "kv24", 70, 130
    cfg, gs, _, body = bc.model(name)
    w, toks = weights(name), bc.tokens(name)
    src = fresh(gpu, cfg, w, toks[:n_pos])
    K, V = caches(src, cfg)
    m = ref_q8.Q8Model(cfg, ck.v2_carve(cfg, body, True, gs), gs, "f64")
    m.kc, m.vc = (kv8_cases.Kv8Rows(m.kc.shape, cfg.head_size, m.ft) for _ in range(2))
    for l in range(cfg.n_layers):
        for t in range(n_pos):
            m.kc[l, t], m.vc[l, t] = K[l, t], V[l, t]
    deep = gpu.RunState(cfg, kv8=True)
    gpu.runstate_fork(deep, src, n_pos)
    shallow = [gpu.RunState(cfg, kv8=True) for _ in range(16)]
    bad = []
    for p in range(n_pos, last + 1):
        gpu.transformer_wide_q8([deep] + shallow, [int(toks[p])] + [int(toks[p - n_pos + i]) for i in range(16)],
                                [p] + [p - n_pos] * 16, w, want_next=False)
        got, want = deep.logits(), m.transformer(int(toks[p]), p)
        if not q8_cases.parity_ok(got, want):
            bad.append((p, q8_cases.scaled_dev(got, want)))
    for s in [src, deep] + shallow:
        s.close()
    print(f"steps over the parity bar (position, deviation of the scale): {bad}")
    assert len(bad) <= (last + 1 - n_pos) // 12 and all(dev <= q8_cases.LOOSE for _, dev in bad)
