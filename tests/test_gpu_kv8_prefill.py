"""The prompt pass straight into int8 KV rows (l2z_prefill_kv8, l2z_kv8_prefill_attention) on the GPU: 1. the
attention against float64, both forms, stale rows poisoned; 2. the written rows bit for bit, and no other; 3. the row form
equals stepping in every byte; 4. the whole pass on the matrix-core form against float64 with int8 rows
(tests/kv8_prefill_cases.py); and the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_prefill_cases as pc  # noqa: E402
import q8_cases  # noqa: E402
import ref_q8  # noqa: E402
from test_gpu_kv8 import raw, same_raw  # noqa: E402
from test_gpu_q8_batch import caches, same  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
S_KERNEL = 200   # no multiple of 64: the last tile is clamped to the last row


# ---------------------------------------------------------------- 1. the kernel against float64
def kernel_inputs(H, KVH, hs, pos0, P, fill):
    """test_gpu_kv8.kernel_inputs' two fills over ONE sequence's rows and P queries"""
    rng, S, last = np.random.default_rng(H * 1000 + hs + len(fill) + pos0), S_KERNEL, pos0 + P - 1
    q = rng.standard_normal((P, H * hs)).astype(f32)
    if fill == "random":   # scales over four decades
        k8, v8 = (rng.integers(-127, 128, (KVH, S, hs)).astype(np.int8) for _ in range(2))
        ks, vs = ((10.0 ** rng.uniform(-5, -1, (KVH, S))).astype(f32) for _ in range(2))
    else:   # the bytes at their ends, zero rows with scale 0, and for every query one key 80 above the rest
        sgn = np.where(rng.random((KVH, hs)) < 0.5, -1, 1)
        q = (np.abs(q).reshape(P, KVH, H // KVH, hs) * sgn[None, :, None, :]).reshape(P, H * hs).astype(f32)
        k8, v8 = (rng.choice(np.array([-128, -127, 127], np.int8), (KVH, S, hs)) for _ in range(2))
        mass = np.abs(q).reshape(P, KVH, H // KVH, hs).sum(axis=3).min(axis=(0, 2))   # the least sum |q| of a kv head's queries
        top = (80.0 * np.sqrt(hs) / (127.0 * mass)).astype(f32)
        ks = np.repeat((top / 100)[:, None], S, axis=1).astype(f32)
        vs = np.full((KVH, S), 0.01, f32)
        k8[:, 2::5], ks[:, 2::5] = 0, 0.0
        v8[:, 3::7], vs[:, 3::7] = 0, 0.0
        for t, scale in ((1, 1.0), (pos0 + P // 2, 2.0)):   # the second one, twice as high, for the queries from it on
            k8[:, t], ks[:, t] = 127 * sgn, scale * top
    ks[:, last + 1:], vs[:, last + 1:] = np.nan, np.nan   # a tile is loaded whole: rows beyond the call's last position ARE read
    return q, k8, ks, v8, vs


def attention64(q, pos0, k8, ks, v8, vs, H):
    P, (KVH, _, hs) = len(q), k8.shape
    out = np.zeros(q.shape)
    for i in range(P):
        T = pos0 + i + 1
        for h in range(H):
            g = h // (H // KVH)
            K, V = (a[g, :T].astype(np.float64) * b[g, :T, None].astype(np.float64) for a, b in ((k8, ks), (v8, vs)))
            s = K @ q[i, h * hs:(h + 1) * hs].astype(np.float64) / np.sqrt(hs)
            e = np.exp(s - s.max())
            out[i, h * hs:(h + 1) * hs] = (e / e.sum()) @ V
    return out


SPANS = [(0, 33), (0, 64), (0, 65), (37, 100), (64, 33), (130, 70)]
FLASH_SHAPES, ROW_SHAPES = [(3, 2, 1, 64), (3, 2, 2, 128), (3, 4, 1, 128)], [(1, 6, 6, 48), (1, 2, 1, 16)]
# the row form in two slices of its 128-row launches, the second one's rows starting inside a segment of 64 keys
ROW_SPANS = SPANS + [(0, 150), (20, 140)]
# the matrix-core form in four query tiles, the last key tile clamped at S_KERNEL
FLASH_SPANS = SPANS + [(0, 200)]
KERNEL_CASES = [shape + span for shape in FLASH_SHAPES for span in FLASH_SPANS] + [shape + span for shape in ROW_SHAPES for span in ROW_SPANS]


@pytest.mark.parametrize("fill", ["random", "adversarial"])
@pytest.mark.parametrize("form,H,KVH,hs,pos0,P", KERNEL_CASES)
def test_the_attention_meets_the_parity_bar_against_float64(gpu, form, H, KVH, hs, pos0, P, fill):
    q, k8, ks, v8, vs = kernel_inputs(H, KVH, hs, pos0, P, fill)
    want = attention64(q, pos0, k8, ks, v8, vs, H)
    got = gpu.kv8_prefill_attention(form, q, pos0, k8, ks, v8, vs, H)
    err = np.abs(got.astype(np.float64) - want)
    print(f"form {form} heads {H}/{KVH} head_size {hs} pos0 {pos0} P {P} {fill}: largest |got - ref| {err.max():.3e}, of the bar "
          f"{(err / (q8_cases.PARITY_ATOL + q8_cases.PARITY_RTOL * np.abs(want))).max():.3f}")
    assert np.all(np.isfinite(got)) and np.all(err <= q8_cases.PARITY_ATOL + q8_cases.PARITY_RTOL * np.abs(want))
    # ... and beyond a query's OWN position inside the last tile: the last ten keys' scales poisoned, the queries before them
    # give the same bits as above (which met float64) -- a mask that multiplied by zero would give NaN.  The last ten queries
    # of this second call see poisoned keys of their own, rightly hold NaN, and are not looked at
    ks[:, pos0 + P - 10:], vs[:, pos0 + P - 10:] = np.nan, np.nan
    same(gpu.kv8_prefill_attention(form, q, pos0, k8, ks, v8, vs, H)[:P - 10], got[:P - 10], "queries before the poisoned keys")


# ---------------------------------------------------------------- the models of tests 2 - 4
@pytest.fixture(scope="module")
def models(gpu):
    """name -> (cfg, weights, tokens): the head_size 64 shape ("hs64") and tests/q8_cases.py's, made once"""
    made = {}

    def get(name):
        if name not in made:
            cfg, gs, body = pc.model() if name == "hs64" else (lambda m: (m[0], m[1], m[3]))(q8_cases.model(name))
            toks = pc.tokens() if name == "hs64" else np.random.default_rng(7).integers(2, cfg.vocab_size, 20).astype(np.int32)
            made[name] = (cfg, gpu.Weights.from_q8(cfg, body, True, gs), toks)
        return made[name]
    yield get
    for _, w, _ in made.values():
        w.close()


# ---------------------------------------------------------------- 2. the written rows, bit for bit, and nothing else
@pytest.mark.parametrize("name,n", [("hs64", 100), ("288", 20)])
def test_the_pass_writes_the_rule_s_bytes_and_scales_and_no_other_row(gpu, models, name, n):
    cfg, w, toks = models(name)
    s, twin = gpu.RunState(cfg, kv8=True), gpu.RunState(cfg)
    before = raw(s, cfg)
    s.prefill_kv8(toks[:n], 0, w)
    twin.prefill_q8(toks[:n], 0, w)
    after = raw(s, cfg)
    for rows, got in zip(caches(twin, cfg), after):   # layer 0 does not depend on the attention
        q_want, s_want = ref_q8.quantize_act(rows[0, :n], cfg.head_size)
        np.testing.assert_array_equal(got[0][0][:n].reshape(-1), q_want)
        same(got[0][1][:n].reshape(-1), s_want, "layer 0 scales")
        assert all(np.abs(q_l[:n]).max(axis=1).min() == 127 for q_l, _ in got)   # every layer's rows were written
    same_raw(before, after, "rows from n on", but=np.arange(cfg.seq_len) < n)
    for r in (s, twin):
        r.close()


# ---------------------------------------------------------------- 3. the row form equals stepping, every layer
@pytest.mark.parametrize("name", ["64", "288"])
def test_the_row_form_leaves_the_bytes_of_stepping(gpu, models, name):
    cfg, w, toks = models(name)
    n, beyond = 20, np.arange(cfg.seq_len) >= 20
    whole, parts, stepped = (gpu.RunState(cfg, kv8=True) for _ in range(3))
    whole.prefill_kv8(toks[:n], 0, w)
    parts.prefill_kv8(toks[:7], 0, w)
    parts.prefill_kv8(toks[7:n], 7, w)
    for p in range(n):
        gpu.transformer_wide_q8([stepped], [int(toks[p])], [p], w, want_next=False)
    same_raw(raw(whole, cfg), raw(stepped, cfg), "one call against stepping", but=beyond)
    same_raw(raw(parts, cfg), raw(stepped, cfg), "7 + 13 against stepping", but=beyond)
    z = [r.logits() for r in (whole, parts, stepped)]   # (the classifier launch differs: the parity bar, not bits)
    assert all(q8_cases.parity_ok(z[a], z[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    for r in (whole, parts, stepped):
        r.close()


# ---------------------------------------------------------------- 4. the whole pass on the matrix-core form
def test_the_pass_meets_the_float64_reference_with_int8_rows(gpu, models):
    """70 tokens, then 30 at position 70 (their keys: earlier int8 rows plus their own), then one wide step at position 100;
    the logits after each call and every layer's dequantized rows under the q8 family's rule."""
    cfg, w, toks = models("hs64")
    z_ref, k_ref, v_ref = pc.reference()
    s = gpu.RunState(cfg, kv8=True)
    z = z_ref.copy()   # (positions whose logits no call leaves: the reference's own)
    s.prefill_kv8(toks[:70], 0, w)
    z[69] = s.logits()
    s.prefill_kv8(toks[70:100], 70, w)
    z[99] = s.logits()
    gpu.transformer_wide_q8([s], [int(toks[100])], [100], w, want_next=False)
    z[100] = s.logits()
    k, v = (c[:, :pc.N_REF] for c in caches(s, cfg))
    s.close()
    ok, dev = q8_cases.check_positions(z, k, v, z_ref, k_ref, v_ref, -(-pc.N_REF // 12))
    print(f"positions over the parity bar {list(np.flatnonzero(~ok))}, largest deviation {dev.max():.3e} of the scale")


# ---------------------------------------------------------------- the refusals
@pytest.mark.parametrize("what", ["an f32 runstate", "f32 weights", "a paged runstate", "positions past seq_len"])
def test_a_refusal_enqueues_nothing_and_changes_nothing(gpu, what):
    B = gpu
    cfg, gs, blob, body = q8_cases.model("64")
    w, wf, toks = B.Weights.from_q8(cfg, body, True, gs), B.Weights(cfg, blob, True), q8_cases.tokens("64")
    s, plain, pool = B.RunState(cfg, kv8=True), B.RunState(cfg), B.KvPool(cfg, 4)
    paged = B.RunState(cfg, pool=pool)
    s.prefill_kv8(toks[:7], 0, w)
    calls = {"an f32 runstate": (lambda: plain.prefill_kv8(toks[:3], 0, w), B.ERR_INVALID),
             "f32 weights": (lambda: s.prefill_kv8(toks[7:10], 7, wf), B.ERR_INVALID),
             "a paged runstate": (lambda: paged.prefill_kv8(toks[:3], 0, w), B.ERR_INVALID),
             "positions past seq_len": (lambda: s.prefill_kv8(toks[:3], cfg.seq_len - 2, w), B.ERR_STATE)}
    before = (raw(s, cfg), s.logits(), plain.logits(), paged.pages())
    with pytest.raises(B.L2ZError) as e:
        calls[what][0]()
    assert e.value.code == calls[what][1], e.value
    same_raw(before[0], raw(s, cfg), what)
    same(before[1], s.logits(), what)
    same(before[2], plain.logits(), what)
    np.testing.assert_array_equal(before[3], paged.pages())
    for r in (s, plain, paged, pool, w, wf):
        r.close()
