"""Speculative verify over int8 KV rows (l2z_verify_kv8, l2z_kv8_verify_attention) on the GPU: 1. the attention
bit for bit against the row form; 2. against float64, rows beyond a query's own position poisoned; 3. one call of 16 rows
leaves the bytes and logits of stepping; 4. draft invariance and the verdict; 5. the draw; 6. the whole pass against float64;
7. the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_prefill_cases as pc  # noqa: E402
import q8_cases  # noqa: E402
from test_gpu_kv8 import raw, same_raw  # noqa: E402
from test_gpu_kv8_prefill import attention64, kernel_inputs  # noqa: E402
from test_gpu_q8_batch import caches, same  # noqa: E402

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2, 16), (6, 6, 48), (4, 1, 128), (2, 1, 64), (1, 1, 256)]
SPANS = [(0, 1), (0, 16), (5, 3), (60, 9), (63, 2), (64, 16), (130, 16)]
KERNEL_CASES = [shape + span for shape in SHAPES for span in SPANS]
P0, N = 5, 16   # the stepped twin: a prompt of P0 tokens, then N greedy steps


# ---------------------------------------------------------------- 1. the kernel, bits
@pytest.mark.parametrize("fill", ["random", "adversarial"])
@pytest.mark.parametrize("H,KVH,hs,pos0,n", KERNEL_CASES)
def test_a_row_has_the_bits_of_the_one_row_kernel(gpu, H, KVH, hs, pos0, n, fill):
    q, k8, ks, v8, vs = kernel_inputs(H, KVH, hs, pos0, n, fill)   # (scales beyond the last position: NaN, never read)
    got = gpu.kv8_verify_attention(q, pos0, k8, ks, v8, vs, H)
    same(got, gpu.kv8_prefill_attention(1, q, pos0, k8, ks, v8, vs, H), "every row")


# ---------------------------------------------------------------- 2. the kernel, float64
@pytest.mark.parametrize("fill", ["random", "adversarial"])
@pytest.mark.parametrize("H,KVH,hs,pos0,n", KERNEL_CASES)
def test_the_attention_meets_the_parity_bar_against_float64(gpu, H, KVH, hs, pos0, n, fill):
    q, k8, ks, v8, vs = kernel_inputs(H, KVH, hs, pos0, n, fill)
    want = attention64(q, pos0, k8, ks, v8, vs, H)
    got = gpu.kv8_verify_attention(q, pos0, k8, ks, v8, vs, H)
    err = np.abs(got.astype(np.float64) - want)
    print(f"heads {H}/{KVH} head_size {hs} pos0 {pos0} n {n} {fill}: largest |got - ref| {err.max():.3e}, of the bar "
          f"{(err / (q8_cases.PARITY_ATOL + q8_cases.PARITY_RTOL * np.abs(want))).max():.3f}")
    assert np.all(np.isfinite(got)) and np.all(err <= q8_cases.PARITY_ATOL + q8_cases.PARITY_RTOL * np.abs(want))
    m = min(3, n - 1)   # the last m keys' scales poisoned: the rows before them keep their bits
    ks[:, pos0 + n - m:], vs[:, pos0 + n - m:] = np.nan, np.nan
    same(gpu.kv8_verify_attention(q, pos0, k8, ks, v8, vs, H)[:n - m], got[:n - m], "rows before the poisoned keys")


# ---------------------------------------------------------------- the models and the stepped twin of tests 3 - 5
@pytest.fixture(scope="module")
def stepped(gpu):
    """name -> (cfg, weights, prompt, fed, z, rows): a kv8 twin given `prompt`, then stepped greedily with
    transformer_wide_q8 through `fed` (fed[i] at position P0 + i, z[i] the logits behind it); rows: raw() of the twin"""
    made = {}

    def get(name):
        if name not in made:
            cfg, gs, _, body = q8_cases.model(name)
            w = gpu.Weights.from_q8(cfg, body, True, gs)
            prompt = np.random.default_rng(7).integers(2, cfg.vocab_size, P0).astype(np.int32)
            twin = gpu.RunState(cfg, kv8=True)
            twin.prefill_kv8(prompt, 0, w)
            fed, z = [], []
            for i in range(N):
                fed.append(int(np.argmax(twin.logits())))
                gpu.transformer_wide_q8([twin], [fed[-1]], [P0 + i], w, want_next=False)
                z.append(twin.logits())
            made[name] = (cfg, w, prompt, np.array(fed, np.int32), z, raw(twin, cfg))
            twin.close()
        return made[name]
    yield get
    for case in made.values():
        case[1].close()


# ---------------------------------------------------------------- 3. stepping identity
@pytest.mark.parametrize("name", ["64", "288"])
def test_one_call_of_16_rows_leaves_the_bytes_and_logits_of_stepping(gpu, stepped, name):
    cfg, w, prompt, fed, z, rows = stepped(name)
    s = gpu.RunState(cfg, kv8=True)
    s.prefill_kv8(prompt, 0, w)
    before, at = raw(s, cfg), np.arange(cfg.seq_len)
    nxt, a = s.verify_kv8(fed, P0, w)
    assert a == N - 1 and [int(t) for t in nxt] == [int(np.argmax(zi)) for zi in z]
    same_raw(raw(s, cfg), rows, "against stepping", but=at >= P0 + N)
    same_raw(raw(s, cfg), before, "rows outside the call", but=(at >= P0) & (at < P0 + N))
    for i in range(N):
        same(s.verify_logits(i), z[i], f"row {i}'s logits")
    s.close()


# ---------------------------------------------------------------- 4. draft invariance and the verdict
@pytest.mark.parametrize("cut,k", [(1, None), (4, None), (16, None), (16, 1), (16, 5)])
def test_ids_logits_and_rows_do_not_depend_on_the_cut_or_the_guesses(gpu, stepped, cut, k):
    cfg, w, prompt, fed, z, rows = stepped("64")
    s, depth, pos = gpu.RunState(cfg, kv8=True), 12, P0
    s.prefill_kv8(prompt, 0, w)
    while pos < P0 + depth:
        t = fed[pos - P0:min(pos - P0 + cut, depth)].copy()
        planted = k is not None and pos == P0
        if planted:
            t[k] = 2 + (t[k] - 1) % (cfg.vocab_size - 2)   # another token of the vocabulary
        nxt, a = s.verify_kv8(t, pos, w)
        assert a == (k - 1 if planted else len(t) - 1)
        assert [int(x) for x in nxt] == [int(np.argmax(s.verify_logits(i))) for i in range(len(t))]
        same(s.logits(), s.verify_logits(a), "the runstate's logits are row a's")
        pos += a + 1
    same_raw(raw(s, cfg), rows, "against the unspeculated twin", but=np.arange(cfg.seq_len) >= P0 + depth)
    same(s.logits(), z[depth - 1], "final logits")
    s.close()


def test_speculate_q8_on_a_kv8_runstate_emits_the_same_ids_whatever_k(gpu):
    cfg, gs, body = q8_cases.peaked_model()
    w, runs = gpu.Weights.from_q8(cfg, body, False, gs), []
    for k in (0, 4, 15):
        s = gpu.RunState(cfg, kv8=True)
        runs.append((gpu.speculate_q8(s, w, q8_cases.GREEDY_PROMPT, q8_cases.GREEDY_STEPS, k)[0], s.logits()))
        s.close()
    for ids, zl in runs[1:]:
        np.testing.assert_array_equal(ids, runs[0][0])
        same(zl, runs[0][1], "final logits")
    w.close()


# ---------------------------------------------------------------- 5. the draw
def test_a_sampled_call_draws_what_sample_batch_draws_from_the_row_s_logits(gpu, stepped):
    cfg, w, prompt, fed, z, rows = stepped("64")
    s, spare = gpu.RunState(cfg, kv8=True), gpu.RunState(cfg)
    s.prefill_kv8(prompt, 0, w)
    coins = gpu.coin_stream(5, N)
    nxt, a = s.verify_kv8(fed, P0, w, 0.8, 0.9, coins)
    for i in range(N):
        spare.write_logits(s.verify_logits(i))
        assert int(nxt[i]) == int(gpu.sample_batch([spare], 0.8, 0.9, coins[i])[0]), f"row {i}"
    assert a == next((i for i in range(N - 1) if fed[i + 1] != nxt[i]), N - 1)
    for r in (s, spare):
        r.close()


# ---------------------------------------------------------------- 6. the whole pass against float64
def test_the_pass_meets_the_float64_reference_with_int8_rows(gpu):
    """70 prompt tokens, then 16 true tokens at 70 and 14 at 86 through verify_kv8: the 30 rows' logits and every layer's
    dequantized rows under the q8 family's rule, as test_gpu_kv8_prefill.py holds the prompt pass to it."""
    cfg, gs, body = pc.model()
    w, toks, s = gpu.Weights.from_q8(cfg, body, True, gs), pc.tokens(), gpu.RunState(cfg, kv8=True)
    z_ref, k_ref, v_ref = pc.reference()
    z = z_ref.copy()   # (positions whose logits no call leaves: the reference's own)
    s.prefill_kv8(toks[:70], 0, w)
    z[69] = s.logits()
    for p0, n in ((70, 16), (86, 14)):
        s.verify_kv8(toks[p0:p0 + n], p0, w)
        for i in range(n):
            z[p0 + i] = s.verify_logits(i)
    gpu.transformer_wide_q8([s], [int(toks[100])], [100], w, want_next=False)   # (the wide step goes on from there)
    z[100] = s.logits()
    k, v = (c[:, :pc.N_REF] for c in caches(s, cfg))
    ok, dev = q8_cases.check_positions(z, k, v, z_ref, k_ref, v_ref, -(-pc.N_REF // 12))
    print(f"positions over the parity bar {list(np.flatnonzero(~ok))}, largest deviation {dev.max():.3e} of the scale")
    for r in (s, w):
        r.close()


# ---------------------------------------------------------------- 7. the refusals
@pytest.mark.parametrize("what", ["an f32 runstate", "f32 weights", "a paged runstate", "17 rows", "positions past seq_len",
                                  "a token outside the vocabulary", "a temperature without coins"])
def test_a_refusal_enqueues_nothing_and_changes_nothing(gpu, stepped, what):
    B = gpu
    cfg, w, prompt, fed, z, rows = stepped("64")
    wf = B.Weights(cfg, q8_cases.model("64")[2], True)
    s, plain, pool = B.RunState(cfg, kv8=True), B.RunState(cfg), B.KvPool(cfg, 4)
    paged = B.RunState(cfg, pool=pool)
    s.prefill_kv8(prompt, 0, w)
    bad = fed[:3].copy()
    bad[1] = cfg.vocab_size
    calls = {"an f32 runstate": (lambda: plain.verify_kv8(fed[:3], 0, w), B.ERR_INVALID),
             "f32 weights": (lambda: s.verify_kv8(fed[:3], P0, wf), B.ERR_INVALID),
             "a paged runstate": (lambda: paged.verify_kv8(fed[:3], 0, w), B.ERR_INVALID),
             "17 rows": (lambda: s.verify_kv8(np.resize(fed, 17), P0, w), B.ERR_INVALID),
             "positions past seq_len": (lambda: s.verify_kv8(fed[:3], cfg.seq_len - 2, w), B.ERR_STATE),
             "a token outside the vocabulary": (lambda: s.verify_kv8(bad, P0, w), B.ERR_STATE),
             "a temperature without coins": (lambda: s.verify_kv8(fed[:3], P0, w, 0.8, 0.9, None), B.ERR_INVALID)}
    before = (raw(s, cfg), s.logits(), plain.logits(), paged.pages())
    with pytest.raises(B.L2ZError) as e:
        calls[what][0]()
    assert e.value.code == calls[what][1], e.value
    same_raw(before[0], raw(s, cfg), what)
    same(before[1], s.logits(), what)
    same(before[2], plain.logits(), what)
    np.testing.assert_array_equal(before[3], paged.pages())
    s.verify_kv8(fed, P0, w)   # ... and the sequence goes on like an undisturbed twin
    same_raw(raw(s, cfg), rows, "going on", but=np.arange(cfg.seq_len) >= P0 + N)
    same(s.logits(), z[N - 1], "going on")
    for r in (s, plain, paged, pool, wf):
        r.close()
