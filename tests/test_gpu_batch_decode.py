"""The batched decode step (l2z_transformer_batch / l2z_argmax_batch) on the GPU.

Every sequence of a batch is its own runstate.  A batched step must change each one exactly as l2z_transformer(tokens[i],
pos[i]) would: its logits (within the parity bar of tests/test_gpu_parity.py against the CPU oracle's stepped pass), its
KV row pos[i] of every layer (2e-5), and no other cache row (bit for bit).  A sequence's logits and KV rows are
bit-identical whatever batch it runs in (size, order, companions).
"""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOGIT_RTOL = 5e-5
LOGIT_ATOL = 5e-5
KV_TOL = 2e-5
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NS = (1, 2, 3, 7, 16)


def pool_positions(seq_len):
    """16 positions: the edges and a long context first, then short ones (the oracle's stepped histories stay cheap)"""
    head = [0, 1, 17, min(300, seq_len - 2), seq_len - 1]
    return head + [p % seq_len for p in range(2, 13)]


class Seq:
    """one sequence: its GPU runstate with the history fed, the token of the batched step, and the oracle's answer"""

    def __init__(self, gpu, cfg, w, pos, rng, use_prefill):
        self.cfg, self.pos = cfg, pos
        self.hist = rng.integers(2, cfg.vocab_size, size=pos).astype(np.int32)
        self.tok = int(rng.integers(2, cfg.vocab_size))
        self.s = gpu.RunState(cfg)
        if pos and use_prefill:
            self.s.prefill(self.hist, 0, w)
        else:
            for p, t in enumerate(self.hist):
                self.s.transformer(int(t), p, w)
        self.s.synchronize()

    def oracle(self, orc, blob, shared):
        m = orc.Model(self.cfg.as_i32(), blob, shared)
        for p, t in enumerate(self.hist):
            m.transformer(int(t), p)
        self.ref = m.transformer(self.tok, self.pos)
        c = self.cfg
        kvd = c.dim // c.n_heads * c.n_kv_heads
        kc = m.state("key_cache", c.n_layers * c.seq_len * kvd).reshape(c.n_layers, c.seq_len, kvd)
        vc = m.state("value_cache", c.n_layers * c.seq_len * kvd).reshape(c.n_layers, c.seq_len, kvd)
        self.ref_k, self.ref_v = kc[:, self.pos].copy(), vc[:, self.pos].copy()
        m.close()


def caches(s, c):
    """the runstate's caches in the reference's order [layer, seq_len, kv_dim] (l2z_runstate_read permutes)"""
    kvd = c.dim // c.n_heads * c.n_kv_heads
    n = c.n_layers * c.seq_len * kvd
    return [s.read(name, 0, n).reshape(c.n_layers, c.seq_len, kvd) for name in ("key_cache", "value_cache")]


def row(cache, pos):
    """KV row `pos` of every layer, [layer, kv_dim]"""
    return cache[:, pos, :]


def check_step(gpu, seqs, w, before):
    """one batched step of `seqs`; every sequence against the oracle, every other cache row bit-unchanged"""
    gpu.transformer_batch([q.s for q in seqs], [q.tok for q in seqs], [q.pos for q in seqs], w)
    out = []
    for q in seqs:
        lg = q.s.logits()
        np.testing.assert_allclose(lg, q.ref, rtol=LOGIT_RTOL, atol=LOGIT_ATOL)
        k, v = caches(q.s, q.cfg)
        np.testing.assert_allclose(row(k, q.pos), q.ref_k, rtol=KV_TOL, atol=KV_TOL)
        np.testing.assert_allclose(row(v, q.pos), q.ref_v, rtol=KV_TOL, atol=KV_TOL)
        k0, v0 = before[id(q)]
        keep = np.ones(q.cfg.seq_len, bool)
        keep[q.pos] = False
        assert np.array_equal(k[:, keep].view(np.uint32), k0[:, keep].view(np.uint32))
        assert np.array_equal(v[:, keep].view(np.uint32), v0[:, keep].view(np.uint32))
        out.append((lg, row(k, q.pos), row(v, q.pos)))
    return out


def run_parity(gpu, orc, cfg, blob, shared, seed):
    w = gpu.Weights(cfg, blob, shared)
    rng = np.random.default_rng(seed)
    seqs = [Seq(gpu, cfg, w, p, rng, use_prefill=(i % 2 == 0)) for i, p in enumerate(pool_positions(cfg.seq_len))]
    with ThreadPoolExecutor(8) as ex:  # the oracle's calls release the GIL
        list(ex.map(lambda q: q.oracle(orc, blob, shared), seqs))
    before = {id(q): caches(q.s, cfg) for q in seqs}
    first = {}
    for n in NS:
        order = rng.permutation(len(seqs))[:n]
        got = check_step(gpu, [seqs[i] for i in order], w, before)
        for i, g in zip(order, got):
            if i in first:  # the same sequence in another batch: the same bits
                for a, b in zip(first[i], g):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (n, i)
            else:
                first[i] = g
    for q in seqs:
        q.s.close()
    w.close()


def golden_models(ck):
    meta = json.load(open(os.path.join(GOLD, "toy_models.json")))
    for ent in meta["models"]:
        c, shared, blob = ck.read_checkpoint(os.path.join(GOLD, ent["checkpoint"]))
        yield ent, c, shared, np.ascontiguousarray(blob, np.float32)


def test_batch_parity_golden_toy_models(gpu, orc, ck):
    """GQA unshared and MHA shared toy checkpoints"""
    for i, (_, c, shared, blob) in enumerate(golden_models(ck)):
        run_parity(gpu, orc, c, blob, shared, seed=10 + i)


@pytest.mark.parametrize("name", ["stories15M", "stories110M", "wide4096"])
def test_batch_parity_model_dims(gpu, orc, ck, name):
    """the stories15M / stories110M dims (110M: seq_len 320 keeps the oracle's histories short) and a 2-layer model
    4096 wide with hidden 11008 (the 7B's matrices)"""
    cfg = {"stories15M": ck.STORIES15M,
           "stories110M": ck.Config(768, 2048, 12, 12, 12, 32000, 320),
           "wide4096": ck.Config(4096, 11008, 2, 32, 32, 512, 64)}[name]
    blob = ck.synth_blob(cfg, True, seed=77)
    run_parity(gpu, orc, cfg, blob, True, seed=20)


def test_batch_golden_greedy(gpu, ck):
    """each toy model's golden prompt greedy-decoded through l2z_transformer_batch + l2z_argmax_batch, in a batch with
    two companions on other prompts: the golden sequence equals tests/golden/*.npz token for token"""
    for ent, c, shared, blob in golden_models(ck):
        exp = np.load(os.path.join(GOLD, ent["expected"]))["tokens"]
        w = gpu.Weights(c, blob, shared)
        prompts = [list(ent["prompt"]), [5, 9], [int(c.vocab_size) - 1, 2, 3, 4]]
        ss = [gpu.RunState(c) for _ in prompts]
        toks = [1] * len(ss)
        outs = [[] for _ in ss]
        for pos in range(len(exp)):
            gpu.transformer_batch(ss, toks, [pos] * len(ss), w)
            am = gpu.argmax_batch(ss)
            for i, p in enumerate(prompts):
                nxt = p[pos] if pos < len(p) else int(am[i])
                outs[i].append(nxt)
                toks[i] = nxt
        assert outs[0] == exp.tolist(), ent["checkpoint"]
        for s in ss:
            s.close()
        w.close()


def test_batch_invariance_bitwise(gpu, ck):
    """a sequence's logits are the same bits alone (n = 1), in a batch of 16 in shuffled orders, and with other
    companions"""
    cfg = ck.STORIES15M
    w = gpu.Weights(cfg, None, True, seed=3)
    rng = np.random.default_rng(5)
    ss = [gpu.RunState(cfg) for _ in range(20)]
    pos = [int(p) for p in rng.integers(0, 40, size=20)]
    toks = [int(t) for t in rng.integers(2, cfg.vocab_size, size=20)]
    for s, p in zip(ss, pos):
        if p:
            s.prefill(rng.integers(2, cfg.vocab_size, size=p).astype(np.int32), 0, w)

    def step(idx):
        gpu.transformer_batch([ss[i] for i in idx], [toks[i] for i in idx], [pos[i] for i in idx], w)
        return {i: ss[i].logits().view(np.uint32).copy() for i in idx}

    alone = {}
    for i in range(20):
        alone.update(step([i]))
    for trial in range(3):
        idx = list(rng.permutation(20)[:16])
        got = step(idx)
        for i in idx:
            assert np.array_equal(got[i], alone[i]), (trial, i)
    for s in ss:
        s.close()
    w.close()


def test_batch_interop_with_prefill_and_single_steps(gpu, orc, ck):
    """l2z_prefill -> batched steps -> l2z_transformer -> batched step on one runstate, against the oracle at every
    step; l2z_probs_read and l2z_argmax right after a batched step; a runstate outside the batch untouched"""
    ent, c, shared, blob = next(golden_models(ck))
    w = gpu.Weights(c, blob, shared)
    m = orc.Model(c.as_i32(), blob, shared)
    rng = np.random.default_rng(9)
    toks = [int(t) for t in rng.integers(2, c.vocab_size, size=12)]
    a, comp, other = gpu.RunState(c), gpu.RunState(c), gpu.RunState(c)
    other.prefill(np.array(toks[:3], np.int32), 0, w)
    k_other, v_other = caches(other, c)
    lg_other = other.logits()
    a.prefill(np.array(toks[:5], np.int32), 0, w)
    for p in range(5):
        ref = m.transformer(toks[p], p)
    np.testing.assert_allclose(a.logits(), ref, rtol=LOGIT_RTOL, atol=LOGIT_ATOL)
    plan = ["batch", "batch", "single", "batch", "single", "batch"]
    for j, how in enumerate(plan):
        p = 5 + j
        ref = m.transformer(toks[p], p)
        if how == "batch":
            gpu.transformer_batch([comp, a], [toks[0], toks[p]], [j, p], w)
            lg = a.logits()
            np.testing.assert_allclose(lg, ref, rtol=LOGIT_RTOL, atol=LOGIT_ATOL)
            e = np.exp((lg - lg.max()).astype(np.float64))
            np.testing.assert_allclose(a.probs(1.0), e / e.sum(), rtol=1e-4, atol=1e-7)
            srt = np.sort(ref)
            if srt[-1] - srt[-2] > 1e-3:
                assert a.argmax() == int(np.argmax(ref))
            assert a.argmax() == int(np.argmax(lg))
        else:
            a.transformer(toks[p], p, w)
            np.testing.assert_allclose(a.logits(), ref, rtol=LOGIT_RTOL, atol=LOGIT_ATOL)
    k2, v2 = caches(other, c)
    assert np.array_equal(k2.view(np.uint32), k_other.view(np.uint32))
    assert np.array_equal(v2.view(np.uint32), v_other.view(np.uint32))
    assert np.array_equal(other.logits().view(np.uint32), lg_other.view(np.uint32))
    for s in (a, comp, other):
        s.close()
    m.close()
    w.close()


def test_batch_contract_violations_change_nothing(gpu, ck):
    """every violation of the contract returns its code with the runstates' caches and logits bit-unchanged"""
    c = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    c2 = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=16)
    w = gpu.Weights(c, None, False, seed=4)
    ss = [gpu.RunState(c) for _ in range(17)]
    for i, s in enumerate(ss):
        s.prefill(np.array([3 + i, 4, 5], np.int32), 0, w)
    foreign = gpu.RunState(c2)
    comm = gpu.Comm(0, 2, None, 0, emulated=True)
    shard = gpu.RunState(c, comm)

    def snap():
        return [(np.concatenate([x.ravel() for x in caches(s, c)]).view(np.uint32), s.logits().view(np.uint32))
                for s in ss]
    before = snap()
    E = gpu.L2ZError
    cases = [
        (ss[:1], [1], [3], gpu.ERR_INVALID, "n = 0", 0),
        (ss, [1] * 17, [3] * 17, gpu.ERR_INVALID, "n = 17", None),
        ([ss[0], ss[0]], [1, 1], [3, 3], gpu.ERR_INVALID, "duplicate", None),
        ([ss[0], foreign], [1, 1], [3, 3], gpu.ERR_INVALID, "other config", None),
        ([ss[0], shard], [1, 1], [3, 3], gpu.ERR_INVALID, "shard", None),
        ([ss[0], ss[1]], [1, 1], [3, -1], gpu.ERR_STATE, "pos < 0", None),
        ([ss[0], ss[1]], [1, 1], [3, 32], gpu.ERR_STATE, "pos = seq_len", None),
        ([ss[0], ss[1]], [1, -1], [3, 3], gpu.ERR_STATE, "token < 0", None),
        ([ss[0], ss[1]], [1, 512], [3, 3], gpu.ERR_STATE, "token = vocab", None),
    ]
    import ctypes as C
    L = gpu.lib()
    for states, toks, pos, code, what, n_override in cases:
        n = len(states) if n_override is None else n_override
        arr = (C.c_void_p * max(len(states), 1))(*[s.h for s in states])
        t = np.array(toks, np.int32)
        p = np.array(pos, np.int32)
        rc = L.l2z_transformer_batch(n, t.ctypes.data_as(C.POINTER(C.c_int32)), p.ctypes.data_as(C.POINTER(C.c_int32)),
                                     C.byref(states[0].cfg), arr, w.h)
        assert rc == code, (what, rc)
        if what in ("n = 0", "n = 17", "duplicate", "other config", "shard"):
            out = (C.c_int32 * 17)()
            assert L.l2z_argmax_batch(n, arr, out) == gpu.ERR_INVALID, what
    with pytest.raises(E) as e:  # config that does not match the runstates
        L2 = gpu.L2ZConfig(*[int(v) for v in c2.as_i32()])
        arr = (C.c_void_p * 2)(ss[0].h, ss[1].h)
        t = np.array([1, 1], np.int32)
        gpu._chk(L.l2z_transformer_batch(2, t.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_int32)),
                                         C.byref(L2), arr, w.h))
    assert e.value.code == gpu.ERR_INVALID
    after = snap()
    for (k0, l0), (k1, l1) in zip(before, after):
        assert np.array_equal(k0, k1) and np.array_equal(l0, l1)
    for s in ss + [foreign, shard]:
        s.close()
    comm.close()
    w.close()


def test_batch_7b_shape_against_single_steps(gpu, ck):
    """synthetic full-size 7B weights, n = 4 at positions 0, 5, 1000, 2047: each sequence's batched logits against
    l2z_transformer's at the same position and history (the parity bar)"""
    cfg = ck.LLAMA2_7B
    w = gpu.Weights(cfg, None, False, seed=2024)
    rng = np.random.default_rng(11)
    pos = [0, 5, 1000, 2047]
    ss = [gpu.RunState(cfg) for _ in pos]
    toks = [int(t) for t in rng.integers(2, cfg.vocab_size, size=4)]
    for s, p in zip(ss, pos):
        if p:
            s.prefill(rng.integers(2, cfg.vocab_size, size=p).astype(np.int32), 0, w)
    gpu.transformer_batch(ss, toks, pos, w)
    got = [s.logits() for s in ss]
    am = gpu.argmax_batch(ss)
    for s, p, t, g, a in zip(ss, pos, toks, got, am):
        assert int(a) == int(np.argmax(g))
        s.transformer(t, p, w)
        np.testing.assert_allclose(g, s.logits(), rtol=LOGIT_RTOL, atol=LOGIT_ATOL)
    for s in ss:
        s.close()
    w.close()
