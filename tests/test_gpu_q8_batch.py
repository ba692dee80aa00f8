"""The batched step and the verify pass on int8 group-quantized weights (l2z_transformer_batch_q8, l2z_verify_q8; DESIGN.md
4.25) on the GPU: a. the products of layer 0 bit for bit against the prompt pass's GEMM and its RoPE; b. row independence
of the batched step; c. draft invariance of the verify pass; d. both against the float64 reference of tests/ref_q8.py under
the prompt pass's rule; e. the speculative loop; f. the refusals.  tests/test_q8_batch_cpu.py checks on the CPU what these
rely on; tests/q8_batch_cases.py holds the shared inputs, tests/q8_cases.py the two bars.

The runstate's next position (host_pos) has no reader: what a call leaves of it is held through the calls that follow it in
the loop of test e."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_batch_cases as bc  # noqa: E402
import q8_cases  # noqa: E402
import q8_prefill_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b, what=""):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=str(what))


@pytest.fixture(scope="module")
def weights(gpu):
    """name -> the shape's quantized weights, made once and closed with the module"""
    made = {}

    def get(name):
        if name not in made:
            cfg, gs, _, body = bc.model(name)
            made[name] = gpu.Weights.from_q8(cfg, body, True, gs)
        return made[name]
    yield get
    for w in made.values():
        w.close()


def caches(s, cfg):
    """(K, V) [L, seq_len, kvd]: every row of both caches"""
    L, S, kvd = cfg.n_layers, cfg.seq_len, cfg.kv_dim
    return (s.read("key_cache", 0, L * S * kvd).reshape(L, S, kvd), s.read("value_cache", 0, L * S * kvd).reshape(L, S, kvd))


def fresh(gpu, cfg, w, history):
    """a runstate that holds `history` at positions 0 .. (one prompt pass; none: untouched)"""
    s = gpu.RunState(cfg)
    if len(history):
        s.prefill_q8(history, 0, w)
    return s


# ---------------------------------------------------------------- a. the products of layer 0, bit for bit
@pytest.mark.parametrize("n", [1, 5, 16])
@pytest.mark.parametrize("name", bc.EXACT_SHAPES)
def test_layer_0_products_are_the_gemm_s_and_the_prompt_pass_s_bits(gpu, ck, weights, name, n):
    cfg, gs, _, body = bc.model(name)
    w = weights(name)
    S = cfg.seq_len
    toks = bc.tokens(name, n)
    emb_q, emb_s = w.q8_read("token_embedding_table")
    wv_q, wv_s = w.q8_read("wv", 0)
    rms_att0 = np.ascontiguousarray(ck.v2_carve(cfg, body, True, gs)["rms_att_weight"][0], f32)
    xq, xs = gpu.q8_quantize_rows(bc.embedding_rows(emb_q, emb_s, toks, gs), gs, rms_att0)
    v_want = gpu.q8_gemm(xq, xs, wv_q, wv_s, gs)   # [n, kvd]
    assert np.all(np.abs(v_want).max(axis=1) > 0)

    def k_want(pos):   # the prompt pass's layer-0 K row of each token at its position, on a twin
        twin = gpu.RunState(cfg)
        out = []
        for t, p in zip(toks, pos):
            twin.prefill_q8([int(t)], int(p), w)
            out.append(twin.read("key_cache", int(p) * cfg.kv_dim, cfg.kv_dim))
        twin.close()
        return np.stack(out)

    # the batched step: every row in its own runstate at its own position (row 0 at 0, the last at the cache's last)
    pos = np.array([S - 1] if n == 1 else [i * (S - 1) // (n - 1) for i in range(n)], np.int32)
    states = [gpu.RunState(cfg) for _ in range(n)]
    gpu.transformer_batch_q8(states, toks, pos, w)
    kw = k_want(pos)
    for i, s in enumerate(states):
        K, V = caches(s, cfg)
        same(V[0, pos[i]], v_want[i], f"batch: V row of row {i}")
        same(K[0, pos[i]], kw[i], f"batch: K row of row {i}")
        s.close()
    # the verify pass: consecutive positions of one runstate
    pos0 = min(3, S - n)
    s = gpu.RunState(cfg)
    s.verify_q8(toks, pos0, w)
    K, V = caches(s, cfg)
    kw = k_want(pos0 + np.arange(n))
    for i in range(n):
        same(V[0, pos0 + i], v_want[i], f"verify: V row of row {i}")
        same(K[0, pos0 + i], kw[i], f"verify: K row of row {i}")
    s.close()


# ---------------------------------------------------------------- b. row independence, bit for bit
@pytest.mark.parametrize("name", ["64", "kv24"])
def test_a_sequence_s_step_does_not_depend_on_the_other_rows(gpu, weights, name):
    cfg, gs, _, _ = bc.model(name)
    w = weights(name)
    toks = bc.tokens(name)
    S, V = cfg.seq_len, cfg.vocab_size
    hist, tok, pos = toks[:5], int(toks[5]), 5   # the sequence under test: five positions behind it

    def run(slot, n, others_tok, others_depth):
        """the sequence as row `slot` of n; row i != slot: others_tok[i] at position others_depth[i] behind that many
        positions of its own.  Checks that the call touched nothing it did not name."""
        states, tk, ps = [], [], []
        for i in range(n):
            d = 5 if i == slot else int(others_depth[i])
            states.append(fresh(gpu, cfg, w, hist if i == slot else toks[7:7 + d]))
            tk.append(tok if i == slot else int(others_tok[i]))
            ps.append(pos if i == slot else d)
        bystander = fresh(gpu, cfg, w, toks[:4])
        before = [caches(s, cfg) for s in states + [bystander]]
        z_by = bystander.logits()
        gpu.transformer_batch_q8(states, tk, ps, w)
        for i, s in enumerate(states + [bystander]):
            (k0, v0), (k1, v1) = before[i], caches(s, cfg)
            named = np.zeros(S, bool)
            if i < n:
                named[ps[i]] = True
                assert np.all(np.abs(k1[:, ps[i]]).max(axis=1) > 0) and np.all(k0[:, ps[i]] == 0)
            same(k0[:, ~named], k1[:, ~named], f"K rows the call does not name, runstate {i}")
            same(v0[:, ~named], v1[:, ~named], f"V rows the call does not name, runstate {i}")
        same(bystander.logits(), z_by, "a runstate the call does not name")
        out = (states[slot].logits(),) + caches(states[slot], cfg)
        assert gpu.argmax_batch(states)[slot] == int(np.argmax(out[0]))
        for s in states + [bystander]:
            s.close()
        return out

    rng = np.random.default_rng(7)
    o_tok, o_depth = rng.integers(2, V, 16), rng.integers(0, min(S - 8, 20), 16)
    alone = run(0, 1, o_tok, o_depth)
    assert np.abs(alone[0]).max() > 0
    runs = {f"row {slot} of 16": run(slot, 16, o_tok, o_depth) for slot in (0, 7, 15)}
    runs["other tokens"] = run(7, 16, rng.integers(2, V, 16), o_depth)
    runs["other depths"] = run(7, 16, o_tok, (o_depth + 3) % min(S - 8, 20))
    runs["row 2 of 5"] = run(2, 5, o_tok, o_depth)
    for what, got in runs.items():
        for a, b in zip(alone, got):
            same(a, b, what)


# ---------------------------------------------------------------- c. draft invariance, bit for bit
@pytest.mark.parametrize("name,pos0,n", bc.VERIFY_CASES)
def test_n_rows_in_one_call_are_n_calls_of_one_row(gpu, weights, name, pos0, n):
    cfg, gs, _, _ = bc.model(name)
    w = weights(name)
    toks = bc.tokens(name)
    hist, rows = toks[:pos0], toks[pos0:pos0 + n]
    V = cfg.vocab_size
    one = fresh(gpu, cfg, w, hist)
    nxt, acc = one.verify_q8(rows, pos0, w)
    z = [one.verify_logits(i) for i in range(n)]
    # the verdict: the first guess that is not the row before's next id
    want = 0
    while want + 1 < n and rows[want + 1] == nxt[want]:
        want += 1
    assert acc == want
    same(one.logits(), z[acc], "the runstate's logits are row `accepted`")
    assert one.argmax() == nxt[acc] == int(np.argmax(z[acc]))
    step = fresh(gpu, cfg, w, hist)
    for i in range(n):
        n1, a1 = step.verify_q8(rows[i:i + 1], pos0 + i, w)
        assert a1 == 0 and n1[0] == nxt[i], f"row {i}"
        same(step.verify_logits(0), z[i], f"logits of row {i}")
        same(step.logits(), z[i], f"logits of row {i}")
    for a, b, what in zip(caches(one, cfg), caches(step, cfg), "KV"):
        same(a[:, :pos0 + n], b[:, :pos0 + n], f"{what} rows")
    one.close()
    # the model's own continuation, row by row; then it guessed right up to row m and wrong there
    cont, zc = [int(rows[0])], []
    ref = fresh(gpu, cfg, w, hist)
    for i in range(n):
        n1, _ = ref.verify_q8([cont[i]], pos0 + i, w)
        zc.append(ref.logits())
        cont.append(int(n1[0]))
    m = max(1, n // 2)
    guess = cont[:n]
    if m < n:
        guess[m] = cont[m] + 1 if cont[m] + 1 < V else 2
    g = fresh(gpu, cfg, w, hist)
    nxt, acc = g.verify_q8(guess, pos0, w)
    assert acc == m - 1 and list(nxt[:m]) == cont[1:m + 1]
    same(g.logits(), zc[m - 1], "the logits behind the last accepted row")
    assert g.argmax() == cont[m]
    for a, b, what in zip(caches(g, cfg), caches(ref, cfg), "KV"):
        same(a[:, :pos0 + m], b[:, :pos0 + m], f"{what} rows up to the last accepted one")
    for s in (step, ref, g):
        s.close()


def test_a_scratch_re_made_for_another_group_size_equals_a_fresh_one(gpu):
    """The step's quantized rows and scales live in the runstate that is states[0]: weights of the same config at another
    group size re-make them, and the runstate then computes what a fresh one computes."""
    import q8_prefill_long_cases as lc
    toks = bc.tokens("wide80", 6)
    got = {}
    used = None
    for gs in (64, 32, 64):
        cfg, _, _, body = lc.model("wide80", gs=gs)
        w = gpu.Weights.from_q8(cfg, body, True, gs)
        used = used or gpu.RunState(cfg)
        for s, what in ((used, "used"), (gpu.RunState(cfg), "fresh")):
            nxt, _ = s.verify_q8(toks, 0, w)
            gpu.transformer_batch_q8([s], toks[5:6], [6], w)
            got[what] = (nxt, s.logits()) + caches(s, cfg)
            if what == "fresh":
                s.close()
        for a, b in zip(got["used"], got["fresh"]):
            same(a[..., :7, :] if a.ndim == 3 else a, b[..., :7, :] if b.ndim == 3 else b, f"group size {gs}")
        w.close()
    used.close()


# ---------------------------------------------------------------- d. against the float64 reference
_flips, _devs = {}, {}


@pytest.mark.parametrize("name", list(bc.REFERENCE_CALLS))
def test_verify_runs_meet_the_float64_reference(gpu, weights, name):
    cfg = bc.model(name)[0]
    w = weights(name)
    toks = pc.tokens(name)
    s = gpu.RunState(cfg)
    z, pos = {}, 0
    for n in bc.REFERENCE_CALLS[name]:
        s.verify_q8(toks[pos:pos + n], pos, w)
        for i in range(n):
            z[pos + i] = s.verify_logits(i)
        pos += n
    k, v = caches(s, cfg)
    s.close()
    flipped, ok, dev = pc.check_rule(z, k[:, :pos], v[:, :pos], pc.reference(name, "f64"))
    print(f"verify, shape {name}: positions over the parity bar {list(np.flatnonzero(~ok))}, largest deviation {dev.max():.3e} of the scale")
    _flips["verify " + name], _devs["verify " + name] = flipped, float(dev.max())


@pytest.mark.parametrize("name", list(bc.REFERENCE_CALLS))
def test_batched_steps_meet_the_float64_reference(gpu, weights, name):
    cfg = bc.model(name)[0]
    w = weights(name)
    feeds = bc.batch_feeds(name)
    P = bc.BATCH_REF_STEPS
    states = [gpu.RunState(cfg) for _ in range(3)]
    solo = gpu.RunState(cfg)
    z = {}
    for p in range(P):
        gpu.transformer_batch_q8(states, feeds[:, p], [p, p, p], w)
        z[p] = states[0].logits()
        gpu.transformer_batch_q8([solo], feeds[1:2, p], [p], w)
        same(states[1].logits(), solo.logits(), f"sequence 1 alone, position {p}")
    k, v = caches(states[0], cfg)
    ref = pc.reference(name, "f64")
    flipped, ok, dev = pc.check_rule(z, k[:, :P], v[:, :P], (ref[0][:P], ref[1][:, :P], ref[2][:, :P]))
    print(f"batch, shape {name}: positions over the parity bar {list(np.flatnonzero(~ok))}, largest deviation {dev.max():.3e} of the scale")
    _flips["batch " + name], _devs["batch " + name] = flipped, float(dev.max())
    for a, b in zip(caches(states[1], cfg), caches(solo, cfg)):
        same(a, b, "sequence 1 alone")
    for s in states + [solo]:
        s.close()


def test_at_most_one_reference_case_left_the_parity_bar():
    """A flipped activation -- a position over the parity bar and under the loose one -- in at most one of the module's
    reference cases that ran: the two CPU modes need none on these runs (tests/test_q8_batch_cpu.py)."""
    flipped = [name for name, f in _flips.items() if f]
    print(f"reference cases run: {sorted(_flips)}, with a position over the parity bar: {flipped}; "
          f"largest deviation {max(_devs.values(), default=0.0):.3e} of the scale")
    assert len(flipped) <= 1


# ---------------------------------------------------------------- e. the loop
def drafters(ids):
    """always wrong, always right (fed the ids the run emits), and the default"""
    V = q8_cases.PEAKED_SHAPE[5]
    ids = [int(t) for t in ids]

    def right(hist, k):
        return ids[len(hist) - 1:len(hist) - 1 + k]

    def wrong(hist, k):
        return [t + 1 if t + 1 < V else 2 for t in right(hist, k)] + [2] * (k - len(right(hist, k)))
    return {"wrong": wrong, "right": right, "lookup": None}


def test_speculate_q8_emits_the_reference_s_ids_whatever_the_draft(gpu):
    ids_ref, margins, zs = q8_cases.peaked_reference()
    assert np.all(margins >= 10 * q8_cases.LOOSE * np.abs(zs).max(axis=1))
    cfg, gs, body = q8_cases.peaked_model()
    w = gpu.Weights.from_q8(cfg, body, False, gs)
    steps = q8_cases.GREEDY_STEPS
    first, accepted = None, {}
    for k in (0, 3, 7):
        for what, drafter in drafters(ids_ref).items():
            s = gpu.RunState(cfg)
            ids, stats = gpu.speculate_q8(s, w, q8_cases.GREEDY_PROMPT, steps, k, drafter)
            np.testing.assert_array_equal(ids, ids_ref, err_msg=f"k {k}, {what}")
            got = (s.logits(),) + tuple(a[:, :steps] for a in caches(s, cfg))
            accepted[(k, what)] = stats["accepted"]
            if first is None:
                first = got
                assert q8_cases.parity_ok(got[0], zs[-1]) or q8_cases.scaled_dev(got[0], zs[-1]) <= q8_cases.LOOSE
            for a, b in zip(first, got):
                same(a, b, f"k {k}, {what}")
            s.close()
    # the drafts were what they were said to be
    assert accepted[(3, "wrong")] == accepted[(7, "wrong")] == 0 and accepted[(7, "right")] > accepted[(3, "right")] > 0
    w.close()


def test_speculate_q8_with_a_temperature_is_coin_invariant(gpu):
    cfg, gs, body = q8_cases.peaked_model()
    w = gpu.Weights.from_q8(cfg, body, False, gs)
    steps = q8_cases.GREEDY_STEPS
    temperature, top_p = 8.0, 0.95   # (the logits are about +22 and -9: at this temperature the top id is drawn at about one step in nine)
    coins = gpu.coin_stream(11, steps)

    def run(k, drafter):
        s = gpu.RunState(cfg)
        ids, stats = gpu.speculate_q8(s, w, q8_cases.GREEDY_PROMPT, steps, k, drafter, temperature, top_p, coins)
        z = s.logits()
        s.close()
        return ids, z, stats

    base, z0, _ = run(0, None)
    assert len(base) > len(q8_cases.GREEDY_PROMPT) and not np.array_equal(base, q8_cases.peaked_reference()[0][:len(base)])
    for k in (3, 7):
        for what, drafter in drafters(base).items():
            ids, z, stats = run(k, drafter)
            np.testing.assert_array_equal(ids, base, err_msg=f"k {k}, {what}")
            same(z, z0, f"k {k}, {what}")
            if what == "right" and len(base) == steps:
                assert stats["accepted"] > 0
    w.close()


# ---------------------------------------------------------------- f. refusals
def test_refusals_enqueue_nothing_and_change_nothing(gpu, ck):
    B = gpu
    cfg, gs, blob, body = q8_cases.model("64")
    w = B.Weights.from_q8(cfg, body, True, gs)
    w32 = B.Weights(cfg, blob, True)
    toks = pc.tokens("64")
    s, s2, twin = B.RunState(cfg), B.RunState(cfg), B.RunState(cfg)
    for r in (s, twin):
        r.prefill_q8(toks[:7], 0, w)
    s2.prefill_q8(toks[:2], 0, w)
    S, kvd, V = cfg.seq_len, cfg.kv_dim, cfg.vocab_size

    def sampled():
        return (s.logits(), s2.logits(), s.read("key_cache", (S + 4) * kvd, kvd), s.read("value_cache", 2 * kvd, kvd),
                s.read("key_cache", 7 * kvd, 3 * kvd), s.read("value_cache", (S + 7) * kvd, 3 * kvd),
                s2.read("key_cache", kvd, 3 * kvd))

    before = sampled()
    pool = B.KvPool(cfg, 4)
    sp = B.RunState(cfg, pool=pool)
    comm = B.Comm(0, 2, None, 0, emulated=True)
    ss = B.RunState(cfg, comm=comm)
    cfg_o, gs_o, _, body_o = q8_cases.model("512")
    so = B.RunState(cfg_o)
    many = [B.RunState(cfg) for _ in range(15)]
    # head sizes of 6 and 512, and a vocabulary of 66: shapes whose objects can be made and the step's launches do not take
    odd = {}
    for what, shp in {"head_size 6": (96, 256, 1, 16, 16, 64, 8), "head_size 512": (1024, 64, 1, 2, 2, 64, 8),
                      "vocab 66": (64, 192, 1, 4, 2, 66, 8)}.items():
        c = ck.Config(*shp)
        wo = B.Weights.from_q8(c, ck.v2_body_from_f32(c, ck.synth_blob(c, True, 3), True, 32), True, 32)
        odd[what] = (wo, B.RunState(c), B.RunState(c))
    three = [7, 8, 9]
    INV, ST = B.ERR_INVALID, B.ERR_STATE
    batch = lambda st, tk, ps, ww=w: (lambda: B.transformer_batch_q8(st, tk, ps, ww))  # noqa: E731
    verify = lambda r, tk, p0, ww=w, **kw: (lambda: r.verify_q8(tk, p0, ww, **kw))  # noqa: E731
    calls = {
        "batch: f32 weights": (batch([s, s2], [7, 8], [7, 2], w32), INV, "l2z_transformer_batch"),
        "batch: a paged runstate": (batch([s, sp], [7, 8], [7, 0]), INV, ""),
        "batch: a sharded runstate": (batch([s, ss], [7, 8], [7, 0]), INV, ""),
        "batch: a foreign config": (batch([s, so], [7, 8], [7, 0]), INV, ""),
        "batch: n = 0": (batch([], [], []), INV, ""),
        "batch: n = 17": (batch([s, s2] + many, [7] * 17, [7, 2] + [0] * 15), INV, ""),
        "batch: the same runstate twice": (batch([s, s], [7, 8], [7, 8]), INV, ""),
        "batch: a position past the cache": (batch([s, s2], [7, 8], [7, S]), ST, ""),
        "batch: a negative position": (batch([s, s2], [7, 8], [-1, 2]), ST, ""),
        "batch: token = vocab_size": (batch([s, s2], [7, V], [7, 2]), ST, ""),
        "batch: head_size 6": (batch(list(odd["head_size 6"][1:]), [7, 8], [0, 0], odd["head_size 6"][0]), INV, "head_size"),
        "batch: head_size 512": (batch(list(odd["head_size 512"][1:]), [7, 8], [0, 0], odd["head_size 512"][0]), INV, "head_size"),
        "verify: head_size 512": (verify(odd["head_size 512"][1], three, 0, odd["head_size 512"][0]), INV, "head_size"),
        "batch: vocab 66": (batch(list(odd["vocab 66"][1:]), [7, 8], [0, 0], odd["vocab 66"][0]), INV, "vocab_size"),
        "verify: f32 weights": (verify(s, three, 7, w32), INV, "l2z_verify"),
        "verify: a paged runstate": (verify(sp, three, 0), INV, ""),
        "verify: a sharded runstate": (verify(ss, three, 0), INV, ""),
        "verify: a foreign config": (verify(so, three, 0), INV, ""),
        "verify: n = 0": (verify(s, [], 7), INV, ""),
        "verify: n = 17": (verify(s, [7] * 17, 7), INV, ""),
        "verify: positions past the cache": (verify(s, three, S - 2), ST, ""),
        "verify: a negative position": (verify(s, three, -1), ST, ""),
        "verify: token = vocab_size": (verify(s, [7, V, 9], 7), ST, ""),
        "verify: head_size 6": (verify(odd["head_size 6"][1], three, 0, odd["head_size 6"][0]), INV, "head_size"),
        "verify: vocab 66": (verify(odd["vocab 66"][1], three, 0, odd["vocab 66"][0]), INV, "vocab_size"),
        "verify: a negative temperature": (verify(s, three, 7, temperature=-1.0, coins=[0.1, 0.2, 0.3]), INV, "temperature"),
        "verify: a temperature that is no number": (verify(s, three, 7, temperature=float("nan"), coins=[0.1, 0.2, 0.3]), INV, "temperature"),
        "verify: top_p above 1": (verify(s, three, 7, temperature=1.0, top_p=1.5, coins=[0.1, 0.2, 0.3]), INV, "top_p"),
        "verify: no coins at a temperature": (verify(s, three, 7, temperature=1.0), INV, "coins"),
        "verify: a coin of 1": (verify(s, three, 7, temperature=1.0, coins=[0.1, 1.0, 0.3]), INV, "coins"),
    }
    for what, (call, code, word) in calls.items():
        with pytest.raises(B.L2ZError) as e:
            call()
        assert e.value.code == code, f"{what}: {e.value}"
        assert word in str(e.value), f"{what}: {e.value}"
    for i, (a, b) in enumerate(zip(before, sampled())):
        same(a, b, f"sample {i}")
    # ... and the next position: the sequence goes on exactly as its undisturbed twin's
    for r in (s, twin):
        r.transformer(int(toks[7]), 7, w)
    same(s.logits(), twin.logits())
    assert s.argmax() == twin.argmax()
    # the f32 entry points still refuse such weights
    for call in (lambda: B.transformer_batch([s, s2], [7, 8], [8, 2], w), lambda: s.verify(three, 8, w)):
        with pytest.raises(B.L2ZError) as e:
            call()
        assert e.value.code == INV
    for wo, a, b in odd.values():
        a.close(); b.close(); wo.close()
    sp.close(); pool.close(); ss.close(); comm.close(); so.close()
    for r in [s, s2, twin] + many:
        r.close()
    w.close(); w32.close()
