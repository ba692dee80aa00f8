"""The int8 KV cache's runstates on the GPU: who refuses such a runstate, and who takes it."""
import numpy as np
import pytest

REFUSED = ["l2z_transformer", "l2z_prefill", "l2z_prefill_q8", "l2z_transformer_batch_q8", "l2z_verify_q8", "l2z_transformer_wide",
           "l2z_step_mixed", "l2z_score", "fork into an f32 runstate", "fork into a paged runstate", "fork from a paged runstate",
           "a mixed-kind call"]


@pytest.mark.gpu
@pytest.mark.parametrize("what", REFUSED)
def test_a_refusal_enqueues_nothing_and_changes_nothing(gpu, what):
    import q8_cases
    from test_gpu_kv8 import fresh8, raw, same, same_raw
    B = gpu
    cfg, gs, blob, body = q8_cases.model("64")
    w, wf, toks = B.Weights.from_q8(cfg, body, True, gs), B.Weights(cfg, blob, True), [int(t) for t in q8_cases.tokens("64")]
    s, s2, twin, plain = fresh8(B, cfg, w, toks[:7]), fresh8(B, cfg, w, toks[:2]), fresh8(B, cfg, w, toks[:7]), B.RunState(cfg)
    pool = B.KvPool(cfg, 4)
    paged = B.RunState(cfg, pool=pool)
    calls = {"l2z_transformer": lambda: s.transformer(toks[7], 7, w),
             "l2z_prefill": lambda: s.prefill(toks[7:10], 7, wf),
             "l2z_prefill_q8": lambda: s.prefill_q8(toks[7:10], 7, w),
             "l2z_transformer_batch_q8": lambda: B.transformer_batch_q8([s, s2], [toks[7], toks[2]], [7, 2], w),
             "l2z_verify_q8": lambda: s.verify_q8(toks[7:10], 7, w),
             "l2z_transformer_wide": lambda: B.transformer_wide([s, s2], [toks[7], toks[2]], [7, 2], wf),
             "l2z_step_mixed": lambda: B.step_mixed([s, s2], [toks[7:10], toks[2:3]], [7, 2], wf),
             "l2z_score": lambda: s.score(toks[7:10], 7, wf),
             "fork into an f32 runstate": lambda: B.runstate_fork(plain, s, 7),
             "fork into a paged runstate": lambda: B.runstate_fork(paged, s, 7),
             "fork from a paged runstate": lambda: B.runstate_fork(s, paged, 0),
             "a mixed-kind call": lambda: B.transformer_wide_q8([s, plain], [toks[7], toks[0]], [7, 0], w)}
    before = (raw(s, cfg), raw(s2, cfg), s.logits(), s2.logits(), plain.logits(), paged.pages())
    with pytest.raises(B.L2ZError) as e:
        calls[what]()
    assert e.value.code == B.ERR_INVALID, e.value
    after = (raw(s, cfg), raw(s2, cfg), s.logits(), s2.logits(), plain.logits(), paged.pages())
    same_raw(before[0], after[0], what)
    same_raw(before[1], after[1], what)
    for a, b in zip(before[2:5], after[2:5]):
        same(a, b, what)
    np.testing.assert_array_equal(before[5], after[5])
    B.transformer_wide_q8([s, twin], [toks[7]] * 2, [7, 7], w)   # the sequence goes on exactly as its undisturbed twin
    same(s.logits(), twin.logits(), what)
    for r in (s, s2, twin, plain, paged, pool, w, wf):
        r.close()


@pytest.mark.gpu
def test_the_logits_only_calls_take_such_a_runstate(gpu):
    import q8_cases
    from test_gpu_kv8 import fresh8, same
    B = gpu
    cfg, gs, _, body = q8_cases.model("64")
    w, toks = B.Weights.from_q8(cfg, body, True, gs), q8_cases.tokens("64")
    s, s2 = fresh8(B, cfg, w, toks[:5]), fresh8(B, cfg, w, toks[:3])
    nxt = B.transformer_wide_q8([s, s2], [int(toks[5]), int(toks[3])], [5, 3], w)
    z = s.logits()
    assert nxt[0] == s.argmax() == int(np.argmax(z)) and list(B.argmax_batch([s, s2])) == list(nxt)
    np.testing.assert_allclose(s.probs(1.0).sum(), 1.0, rtol=1e-5)
    assert list(B.sample_batch([s, s2], 0.0, 1.0, [0.5, 0.5])) == list(nxt)
    s.write_logits(z[::-1].copy())
    same(s.logits(), z[::-1], "write_logits")
    s.synchronize()
    assert s.read("x", 0, cfg.dim).shape == (cfg.dim,)
    with pytest.raises(B.L2ZError):
        B.RunState(cfg).read_kv8("k", 0, 0, 1)
    for r in (s, s2, w):
        r.close()
