"""The wide step on int8 group-quantized weights (l2z_transformer_wide_q8) and the register-blocked GEMM form under it
(l2z_q8_gemm_wide) on the GPU: 1. the form against l2z_q8_gemm bit for bit and against float64; 2. layer 0 of
the step bit for bit; 3. row independence; 4. the float64 reference; 5. depth, against the batched step; 6. the loop;
7. the refusals.  The shared inputs are tests/q8_cases.py's, q8_batch_cases.py's and q8_prefill_cases.py's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_batch_cases as bc  # noqa: E402
import q8_cases  # noqa: E402
import ref_q8  # noqa: E402
from test_gpu_q8_batch import caches, fresh, same, weights  # noqa: E402,F401
from test_gpu_q8_prefill import gemm_inputs  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32

# (m, d, n, gs): a block owns 32 weight rows -- d of 4, a tile short of a block, a block, 4 and 36 past one; K of one, two,
# nine, 66 and 172 groups (eight waves, batches of four: waves with no group, with part of a batch, with several batches)
GEMM_CASES = [(17, 4, 64, 64), (17, 36, 64, 32), (33, 16, 288, 32), (33, 32, 288, 32), (100, 36, 288, 32), (100, 32, 4224, 64),
              (128, 68, 4224, 64), (128, 16, 11008, 64)]


@pytest.mark.parametrize("fill", ["random", "extreme"])
@pytest.mark.parametrize("m,d,n,gs", GEMM_CASES)
def test_the_form_has_the_gemm_s_bits_and_meets_the_derived_bound(gpu, m, d, n, gs, fill):
    xq, xs, wq, ws = gemm_inputs(m, d, n, gs, fill)
    got = gpu.q8_gemm_wide(xq, xs, wq, ws, gs)
    same(got, gpu.q8_gemm(xq, xs, wq, ws, gs), "every row")
    G, worst = n // gs, 0.0
    for t in range(m):   # (G + 3) 2^-24 sum |term|: two roundings a term and any order of the f32 sum (tests/test_gpu_q8.py)
        terms = ref_q8.matvec_terms64(wq, ws, xq[t], xs[t], gs)
        err, bound = np.abs(got[t].astype(np.float64) - terms.sum(axis=1)), (G + 3) * 2.0 ** -24 * np.abs(terms).sum(axis=1)
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), f"token {t}: features over the bound: {np.flatnonzero(err > bound)[:8]}"
    print(f"m {m} d {d} n {n} gs {gs} {fill}: worst error / bound {worst:.3f}")
    for bad_m in (16, 129):
        with pytest.raises(gpu.L2ZError):
            gpu.q8_gemm_wide(np.resize(xq, (bad_m, n)), np.resize(xs, (bad_m, G)), wq, ws, gs)


@pytest.mark.parametrize("epi", ["store", "resid", "swiglu"])
@pytest.mark.parametrize("m,d,n,gs", [(17, 40, 288, 32), (33, 32, 4224, 64), (100, 72, 4224, 64), (128, 40, 288, 32)])
def test_every_epilogue_of_the_form_has_the_gemm_s_bits(gpu, m, d, n, gs, epi):
    """One launch of each form with the epilogue the passes give it: NT = 2 and 4, one pass and two, both group sizes, nine
    and 66 groups, a last block of one tile and of a part of one.  The residual epilogue also against res + the store sums."""
    xq, xs, wq, ws = gemm_inputs(m, d, n, gs, "random")
    res = np.random.default_rng(m + d).standard_normal((m, d)).astype(f32)
    got = gpu.q8_gemm_epi(epi, True, xq, xs, wq, ws, gs, res)
    same(got, gpu.q8_gemm_epi(epi, False, xq, xs, wq, ws, gs, res), epi)
    assert got.shape == (m, d // 2 if epi == "swiglu" else d) and np.all(np.abs(got).max(axis=1) > 0)
    if epi == "resid":
        same(got, res + gpu.q8_gemm_wide(xq, xs, wq, ws, gs), "res + product, one rounding")


@pytest.mark.parametrize("n", [17, 128])
@pytest.mark.parametrize("name", bc.EXACT_SHAPES)
def test_layer_0_is_the_gemm_s_and_the_prompt_pass_s_bits(gpu, ck, weights, name, n):
    cfg, gs, _, body = bc.model(name)
    w, S, kvd = weights(name), cfg.seq_len, cfg.kv_dim
    toks = np.resize(bc.tokens(name), n)
    pos = np.array([i * (S - 1) // (n - 1) for i in range(n)], np.int32)
    emb_q, emb_s = w.q8_read("token_embedding_table")
    rms_att0 = np.ascontiguousarray(ck.v2_carve(cfg, body, True, gs)["rms_att_weight"][0], f32)
    xq, xs = gpu.q8_quantize_rows(bc.embedding_rows(emb_q, emb_s, toks, gs), gs, rms_att0)
    v_want = gpu.q8_gemm(xq, xs, *w.q8_read("wv", 0), gs)
    states = [gpu.RunState(cfg) for _ in range(n)]
    nxt = gpu.transformer_wide_q8(states, toks, pos, w)
    twin = gpu.RunState(cfg)
    for i, s in enumerate(states):
        twin.prefill_q8([int(toks[i])], int(pos[i]), w)
        same(s.read("value_cache", int(pos[i]) * kvd, kvd), v_want[i], f"V row of row {i}")
        same(s.read("key_cache", int(pos[i]) * kvd, kvd), twin.read("key_cache", int(pos[i]) * kvd, kvd), f"K row of row {i}")
        assert nxt[i] == s.argmax() == int(np.argmax(s.logits()))
        s.close()
    twin.close()


@pytest.mark.parametrize("name", ["64", "kv24"])
def test_a_sequence_s_step_does_not_depend_on_the_other_rows(gpu, weights, name):
    cfg, w, toks = bc.model(name)[0], weights(name), bc.tokens(name)
    S, V, n, slot = cfg.seq_len, cfg.vocab_size, 17, 9
    rng = np.random.default_rng(7)

    def run(o_tok, o_depth):
        """the sequence (five positions behind it) as row `slot` of n; row i != slot: o_tok[i] behind o_depth[i] positions"""
        depth = [5 if i == slot else int(o_depth[i]) for i in range(n)]
        states = [fresh(gpu, cfg, w, toks[:5] if i == slot else toks[7:7 + depth[i]]) for i in range(n)]
        bystander = fresh(gpu, cfg, w, toks[:4])
        before, z_by = [caches(s, cfg) for s in states], bystander.logits()
        gpu.transformer_wide_q8(states, [int(toks[5]) if i == slot else int(o_tok[i]) for i in range(n)], depth, w, want_next=False)
        for i, s in enumerate(states):
            named = np.arange(S) == depth[i]
            for a, b in zip(before[i], caches(s, cfg)):
                same(a[:, ~named], b[:, ~named], f"cache rows the call does not name, runstate {i}")
                assert np.all(np.abs(b[:, named]).max(axis=2) > 0)
        same(bystander.logits(), z_by, "a runstate the call does not name")
        out = (states[slot].logits(),) + caches(states[slot], cfg)
        for s in states + [bystander]:
            s.close()
        return out

    o_tok, o_depth = rng.integers(2, V, n), rng.integers(0, min(S - 8, 20), n)
    first = run(o_tok, o_depth)
    assert np.abs(first[0]).max() > 0
    for what, got in {"other tokens": run(rng.integers(2, V, n), o_depth), "other depths": run(o_tok, (o_depth + 3) % min(S - 8, 20))}.items():
        for a, b in zip(first, got):
            same(a, b, what)


@pytest.mark.parametrize("n", [17, 128])
@pytest.mark.parametrize("name", list(q8_cases.SHAPES))
def test_the_step_meets_the_float64_reference(gpu, weights, name, n):
    """Sequence j stands at position j mod 12 of the shape's reference run and is fed that position's token; the rows,
    grouped by position, under the family's rule: at most one position in twelve over the parity bar, and under LOOSE."""
    cfg, w, toks, P = q8_cases.model(name)[0], weights(name), q8_cases.tokens(name), q8_cases.N_POS
    states = [fresh(gpu, cfg, w, toks[:j % P]) for j in range(n)]
    gpu.transformer_wide_q8(states, [toks[j % P] for j in range(n)], [j % P for j in range(n)], w, want_next=False)
    z = np.stack([states[p].logits() for p in range(P)])
    k, v = (np.stack([c[:, p] for p, c in enumerate(kv)], axis=1) for kv in zip(*[caches(states[p], cfg) for p in range(P)]))
    for j in range(P, n):   # the same token behind the same history: the same bits whatever the row
        same(states[j].logits(), z[j % P], f"row {j}")
    for s in states:
        s.close()
    ok, dev = q8_cases.check_positions(z, k, v, *q8_cases.reference(name), 1)
    print(f"wide, shape {name}, n {n}: positions over the parity bar {list(np.flatnonzero(~ok))}, largest deviation {dev.max():.3e} of the scale")


def test_deep_rows_are_the_batched_step_s(gpu, weights):
    cfg, w, toks = bc.model("kv24")[0], weights("kv24"), bc.tokens("kv24")
    depth = [0, 63, 64, 65, 130, 159] + [int(d) for d in np.random.default_rng(3).integers(1, 159, 14)]
    wide, twins = ([fresh(gpu, cfg, w, toks[:d]) for d in depth] for _ in range(2))
    tk = [int(toks[d]) for d in depth]
    gpu.transformer_wide_q8(wide, tk, depth, w, want_next=False)
    for at in (0, 16):
        gpu.transformer_batch_q8(twins[at:at + 16], tk[at:at + 16], depth[at:at + 16], w)
    loose = []
    for i, (a, b) in enumerate(zip(wide, twins)):
        for ca, cb, what in zip(caches(a, cfg), caches(b, cfg), "KV"):
            same(ca[0, depth[i]], cb[0, depth[i]], f"layer-0 {what} row of row {i}")
        if not q8_cases.parity_ok(a.logits(), b.logits()):
            loose.append((i, depth[i], q8_cases.scaled_dev(a.logits(), b.logits())))
        a.close(); b.close()
    print(f"rows over the parity bar (row, depth, deviation): {loose}")
    assert len(loose) <= 1 and all(dev <= q8_cases.LOOSE for _, _, dev in loose)


def test_generate_wide_q8_emits_the_reference_s_ids(gpu):
    ids_ref = q8_cases.peaked_reference()[0]
    cfg, gs, body = q8_cases.peaked_model()
    w = gpu.Weights.from_q8(cfg, body, False, gs)
    start = [5 + j % 7 for j in range(17)]   # sequence j: BOS and the walk's first start[j] ids behind it
    got = gpu.generate_wide_q8(cfg, w, [[1] + [int(t) for t in ids_ref[:p]] for p in start], 5)
    for j, p in enumerate(start):
        np.testing.assert_array_equal(got[j], ids_ref[p:p + 5], err_msg=f"sequence {j}")
    w.close()


REFUSALS = ["f32 weights", "a paged runstate beside a contiguous one", "paged runstates", "a sharded runstate", "a foreign config", "n = 0", "n = 129", "the same runstate twice",
            "a position past the cache", "a token outside the vocabulary", "head_size 6", "head_size 512", "vocab 66"]


@pytest.mark.parametrize("what", REFUSALS)
def test_a_refusal_enqueues_nothing_and_changes_nothing(gpu, ck, what):
    B = gpu
    cfg, gs, blob, body = q8_cases.model("64")
    w, toks = B.Weights.from_q8(cfg, body, True, gs), q8_cases.tokens("64")
    s, s2, twin = (fresh(B, cfg, w, toks[:d]) for d in (7, 2, 7))
    S, kvd, V = cfg.seq_len, cfg.kv_dim, cfg.vocab_size
    made, code, word = [], B.ERR_INVALID, ""
    st, tk, ps, ww = [s, s2], [7, 8], [7, 2], w
    if what == "f32 weights":
        ww, word = B.Weights(cfg, blob, True), "l2z_transformer_wide"
        made.append(ww)
    elif what in ("a paged runstate beside a contiguous one", "paged runstates"):
        pool = B.KvPool(cfg, 4)
        made += [B.RunState(cfg, pool=pool), B.RunState(cfg, pool=pool), pool]
        st, ps, word = ([s, made[0]], ps, "") if "beside" in what else (made[:2], [0, 0], "paged")
    elif what == "a sharded runstate":
        comm = B.Comm(0, 2, None, 0, emulated=True)
        st = [s, B.RunState(cfg, comm=comm)]
        made += [st[1], comm]
    elif what == "a foreign config":
        st = [s, B.RunState(q8_cases.model("512")[0])]
        made.append(st[1])
    elif what == "n = 0":
        st, tk, ps = [], [], []
    elif what == "n = 129":
        made += [B.RunState(cfg) for _ in range(127)]
        st, tk, ps = [s, s2] + made, [7] * 129, [7, 2] + [0] * 127
    elif what == "the same runstate twice":
        st = [s, s]
    elif what == "a position past the cache":
        ps, code = [7, S], B.ERR_STATE
    elif what == "a token outside the vocabulary":
        tk, code = [7, V], B.ERR_STATE
    else:   # shapes whose objects can be made and the step's launches do not take
        c = ck.Config(*{"head_size 6": (96, 256, 1, 16, 16, 64, 8), "head_size 512": (1024, 64, 1, 2, 2, 64, 8), "vocab 66": (64, 192, 1, 4, 2, 66, 8)}[what])
        ww = B.Weights.from_q8(c, ck.v2_body_from_f32(c, ck.synth_blob(c, True, 3), True, 32), True, 32)
        st, ps, word = [B.RunState(c), B.RunState(c)], [0, 0], what.split()[0] if "head" in what else "vocab_size"
        made += st + [ww]

    def sampled():
        return (s.logits(), s2.logits(), s.read("key_cache", 7 * kvd, 3 * kvd), s.read("value_cache", (S + 7) * kvd, 3 * kvd),
                s2.read("key_cache", kvd, 3 * kvd))

    before = sampled()
    with pytest.raises(B.L2ZError) as e:
        B.transformer_wide_q8(st, tk, ps, ww)
    assert e.value.code == code and word in str(e.value), e.value
    for a, b in zip(before, sampled()):
        same(a, b, what)
    for r in (s, twin):   # ... and the next position: the sequence goes on exactly as its undisturbed twin's
        r.transformer(int(toks[7]), 7, w)
    same(s.logits(), twin.logits(), what)
    for r in made + [s, s2, twin, w]:
        r.close()
