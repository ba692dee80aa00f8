"""l2z_verify_tree on the GPU: the verify pass for a TREE of guesses on one sequence in one sweep of the weights, its verdict
walk, the compaction of the accepted branch's KV rows, and the loop on top (RunState.verify_tree, binding.speculate_tree).

The references: l2z_verify / l2z_verify_sample themselves on a twin forked at pos0, given the tokens on a node's path as a
chain (PATH INVARIANCE: uint32 compares of logits rows, ids, KV rows and the runstate's logits); the CPU oracle stepped
along each path for values (logits rtol = atol = 5e-5, KV rows 2e-5: the bars of tests/test_gpu_verify.py);
speculate_greedy / speculate_sample and the plain greedy loop for the loops.

Models and streams are tests/test_gpu_verify_batch.py's: toy_gqa_unshared (head_size 16, context 32, GQA), stories15M
(head_size 48: a lane group is not a power-of-two fit), long_gqa (head_size 128, kv_mul 2, context 2048: many segments).
A call at pos0 never touches a cache row below pos0, so ONE runstate and ONE twin serve every call of a case."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_verify import LOGIT_ATOL, LOGIT_RTOL, KV_TOL, bits, caches, feed_history, np_argmax
from test_gpu_verify_batch import DRAWS, Stream

pytestmark = pytest.mark.gpu

SEG = 64  # csrc/batch_decode.h kVerifySeg
NAMES = ("toy_gqa_unshared", "stories15M", "long_gqa")

CHAIN = [-1] + list(range(15))
STAR = [-1] + [0] * 15
# 16 nodes, depth 4, branching at every level; the path 0 - 2 - 3 - 5 - 9 is not the lowest-numbered one at any level, and
# its physical rows (2, 3, 5, 9) all have to move (to 1, 2, 3, 4), row 2 being read for depth 1 and written for depth 2
BUSH = [-1, 0, 0, 2, 1, 3, 3, 4, 2, 5, 5, 6, 7, 8, 0, 1]
BUSH_PATH = [0, 2, 3, 5, 9]


def depths(parent):
    d = []
    for p in parent:
        d.append(0 if p < 0 else d[p] + 1)
    return d


def path_of(parent, i):
    out = []
    while i >= 0:
        out.append(i)
        i = parent[i]
    return out[::-1]


def np_walk(tokens, parent, nxt):
    cur, path = 0, [0]
    while True:
        kids = [c for c in range(len(tokens)) if parent[c] == cur and int(tokens[c]) == int(nxt[cur])]
        if not kids:
            return path
        cur = kids[0]
        path.append(cur)


@pytest.fixture(scope="module")
def streams(ck, orc):
    with ThreadPoolExecutor(len(NAMES)) as ex:  # the oracle's calls release the GIL
        out = dict(zip(NAMES, ex.map(lambda n: Stream(ck, orc, n), NAMES)))
    yield out
    for st in out.values():
        st.m.close()


@pytest.fixture(scope="module")
def weights(gpu, streams):
    out = {n: gpu.Weights(st.cfg, st.blob, st.shared) for n, st in streams.items()}
    yield out
    for w in out.values():
        w.close()


def cases(seq_len):
    """(what, parent, pos0); a shorter context cuts pos0 to fit"""
    out = [("chain", CHAIN, 9), ("star", STAR, 9), ("bush", BUSH, 9), ("bush across 64", BUSH, SEG - 3), ("one node", [-1], 9)]
    if seq_len >= 5 * SEG + 220 + 16:
        out.append(("bush deep", BUSH, 5 * SEG + 220))
    return [(what, par, min(pos0, seq_len - len(par))) for what, par, pos0 in out]


def random_tree_tokens(st, rng, parent, pos0, avoid=()):
    """the stream's token at the root, pairwise different random ids (so siblings differ) elsewhere"""
    c = st.cfg
    pool = np.setdiff1d(np.arange(2, c.vocab_size), np.array(list(avoid), np.int64))
    toks = rng.choice(pool, size=len(parent), replace=False).astype(np.int32)
    toks[0] = st.toks[pos0]
    return toks


def pair(gpu, st, w, pos0, by_verify):
    s = gpu.RunState(st.cfg)
    feed_history(s, w, st.toks, pos0, by_verify)
    t = gpu.RunState(st.cfg)
    gpu.runstate_fork(t, s, pos0)
    return s, t


def kv_row(s, c, pos):
    """cache row `pos` of every layer, keys then values (a small read: the per-node compares do not fetch whole caches)"""
    kvd = c.dim // c.n_heads * c.n_kv_heads
    return np.stack([s.read(name, (l * c.seq_len + pos) * kvd, kvd) for name in ("key_cache", "value_cache")
                     for l in range(c.n_layers)])


# ---- 1. path invariance, bit for bit -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("by_verify", [False, True], ids=["prefill", "verify"])
@pytest.mark.parametrize("name", NAMES)
def test_every_node_is_bitwise_the_chain_call_on_its_path(gpu, streams, weights, name, by_verify):
    st, w = streams[name], weights[name]
    c = st.cfg
    rng = np.random.default_rng(11)
    done = {}
    for what, parent, pos0 in cases(c.seq_len):
        if pos0 not in done:
            done[pos0] = pair(gpu, st, w, pos0, by_verify)
        s, t = done[pos0]
        n, dep = len(parent), depths(parent)
        toks = random_tree_tokens(st, rng, parent, pos0)
        k0 = caches(s, c)
        nxt, path, a = s.verify_tree(toks, parent, pos0, w)
        assert path.tolist() == np_walk(toks, parent, nxt) and a == len(path) - 1, (name, what)
        z = [s.verify_logits(i) for i in range(n)]
        kv = caches(s, c)
        moved = {d for d in range(1, a + 1) if path[d] != d}   # physical rows the compaction wrote
        for i in range(n):
            p = path_of(parent, i)
            tn, _ = t.verify(toks[p], pos0, w)
            assert np.array_equal(bits(t.verify_logits(dep[i])), bits(z[i])), (name, what, "logits of node", i)
            assert int(tn[dep[i]]) == int(nxt[i]) == np_argmax(z[i]), (name, what, "id of node", i)
            if i not in moved:   # node i's K / V sit in physical row pos0 + i, the chain's in row pos0 + depth
                mine = np.stack([x[l, pos0 + i] for x in kv for l in range(c.n_layers)])
                assert np.array_equal(bits(mine), bits(kv_row(t, c, pos0 + dep[i]))), (name, what, "KV of node", i)
        with pytest.raises(gpu.L2ZError):
            s.verify_logits(n)
        keep = np.ones(c.seq_len, bool)
        keep[pos0:pos0 + n] = False
        for x0, x1 in zip(k0, kv):
            assert np.array_equal(bits(x0[:, keep]), bits(x1[:, keep])), (name, what, "rows outside the call")
        assert np.array_equal(bits(s.logits()), bits(z[path[a]]))
        if what == "chain":   # l2z_verify's call: everything the single call leaves
            tn, ta = t.verify(toks, pos0, w)
            assert nxt.tolist() == tn.tolist() and a == ta and path.tolist() == list(range(a + 1))
            assert np.array_equal(bits(s.logits()), bits(t.logits()))
            for mine, theirs in zip(kv, caches(t, c)):
                assert np.array_equal(bits(mine), bits(theirs)), (name, "chain: whole caches")
    for s, t in done.values():
        s.close(); t.close()


def test_head_size_256_is_bitwise_the_chain_call_too(gpu, ck):
    """head_size 256: a lane group is a whole wave, so a block has four groups and the tree's key rows take two rounds (no
    model of the table has that head size; synthetic weights, the twin is the only reference)"""
    c = ck.Config(dim=512, hidden_dim=1376, n_layers=2, n_heads=2, n_kv_heads=1, vocab_size=512, seq_len=128)
    w = gpu.Weights(c, None, False, seed=9)
    rng = np.random.default_rng(12)
    pos0 = SEG - 3
    hist = rng.integers(2, c.vocab_size, size=pos0 + 1).astype(np.int32)
    s, t = gpu.RunState(c), gpu.RunState(c)
    s.prefill(hist[:pos0], 0, w)
    gpu.runstate_fork(t, s, pos0)
    for parent in (BUSH, STAR, CHAIN):
        dep = depths(parent)
        toks = rng.choice(np.arange(2, c.vocab_size), size=len(parent), replace=False).astype(np.int32)
        toks[0] = hist[pos0]
        nxt, path, a = s.verify_tree(toks, parent, pos0, w)
        assert path.tolist() == np_walk(toks, parent, nxt)
        z = [s.verify_logits(i) for i in range(len(parent))]
        for i in range(len(parent)):
            tn, _ = t.verify(toks[path_of(parent, i)], pos0, w)
            assert np.array_equal(bits(t.verify_logits(dep[i])), bits(z[i])), ("logits of node", i)
            assert int(tn[dep[i]]) == int(nxt[i])
            if i > a:
                assert np.array_equal(bits(kv_row(s, c, pos0 + i)), bits(kv_row(t, c, pos0 + dep[i]))), ("KV of node", i)
    s.close(); t.close(); w.close()


# ---- 2. verdict and compaction ---------------------------------------------------------------------------------------------------

def planted(st, rng, parent, route, r, pos0):
    """the oracle's own continuation behind pos0 along route[1 .. r], decoys (no id of that continuation) elsewhere"""
    g = st.chain(pos0, r + 1)   # g[r] is what the model says behind the last planted node: no child may carry it
    toks = random_tree_tokens(st, rng, parent, pos0, avoid=g)
    for d in range(1, r + 1):
        toks[route[d]] = g[d - 1]
    return toks, g


@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("name", NAMES)
def test_planted_branch_is_accepted_and_moved_into_place(gpu, streams, weights, name, r):
    st, w = streams[name], weights[name]
    c = st.cfg
    pos0 = {"toy_gqa_unshared": 7, "stories15M": SEG - 3, "long_gqa": 5 * SEG + 220}[name]
    s, t = pair(gpu, st, w, pos0, by_verify=False)
    # stale rows behind pos0, so that "unchanged" below means something
    s.prefill(st.toks[:min(pos0 + 24, c.seq_len)], 0, w)
    gpu.runstate_fork(t, s, c.seq_len)
    toks, g = planted(st, np.random.default_rng(20 + r), BUSH, BUSH_PATH, r, pos0)
    k0 = caches(s, c)
    nxt, path, a = s.verify_tree(toks, BUSH, pos0, w)
    assert a == r and path.tolist() == BUSH_PATH[:r + 1], (name, path, a)
    assert nxt[path].tolist() == g[:r + 1]
    tn, ta = t.verify(toks[BUSH_PATH[:r + 1]], pos0, w)
    assert ta == r and tn.tolist() == nxt[path].tolist()
    assert np.array_equal(bits(s.logits()), bits(t.logits()))
    sl = slice(pos0, pos0 + r + 1)
    k1 = caches(s, c)
    for mine, theirs in zip(k1, caches(t, c)):
        assert np.array_equal(bits(mine[:, sl]), bits(theirs[:, sl])), (name, "accepted rows")
    keep = np.ones(c.seq_len, bool)
    keep[pos0:pos0 + len(BUSH)] = False
    for x0, x1 in zip(k0, k1):
        assert np.array_equal(bits(x0[:, keep]), bits(x1[:, keep])), (name, "rows outside the call")
    # six further greedy positions through l2z_verify on both
    p, tok_s, tok_t = pos0 + r + 1, int(nxt[path[a]]), int(tn[ta])
    for _ in range(min(6, c.seq_len - p)):
        (ns, _), (nt, _) = s.verify([tok_s], p, w), t.verify([tok_t], p, w)
        assert int(ns[0]) == int(nt[0])
        tok_s, tok_t, p = int(ns[0]), int(nt[0]), p + 1
    for mine, theirs in zip(caches(s, c), caches(t, c)):
        assert np.array_equal(bits(mine[:, :p]), bits(theirs[:, :p])), (name, "rows below the next position")
    assert np.array_equal(bits(s.logits()), bits(t.logits()))
    s.close(); t.close()


# ---- 3. sampled --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_sampled_nodes_are_verify_sample_on_their_paths(gpu, streams, weights, name):
    st, w = streams[name], weights[name]
    c = st.cfg
    pos0 = min(SEG - 3, c.seq_len - len(BUSH))
    s, t = pair(gpu, st, w, pos0, by_verify=False)
    dep = depths(BUSH)
    toks = random_tree_tokens(st, np.random.default_rng(30), BUSH, pos0)
    for j, (temp, top_p) in enumerate(DRAWS):
        coins = gpu.coin_stream(60 + j, max(dep) + 1)
        nxt, path, a = s.verify_tree(toks, BUSH, pos0, w, temp, top_p, None if temp == 0 else coins)
        assert path.tolist() == np_walk(toks, BUSH, nxt) and a == len(path) - 1
        z = [s.verify_logits(i) for i in range(len(BUSH))]
        for i in range(len(BUSH)):
            p = path_of(BUSH, i)
            tn, _ = t.verify_sample(toks[p], pos0, w, temp, top_p, None if temp == 0 else coins[:dep[i] + 1])
            assert int(tn[dep[i]]) == int(nxt[i]), (name, temp, top_p, "node", i)
            assert np.array_equal(bits(t.verify_logits(dep[i])), bits(z[i]))
        if temp == 0:   # no coins at temperature 0: the greedy call
            n0, p0, a0 = s.verify_tree(toks, BUSH, pos0, w)
            assert n0.tolist() == nxt.tolist() and p0.tolist() == path.tolist() and a0 == a
            for i in range(len(BUSH)):
                assert np.array_equal(bits(s.verify_logits(i)), bits(z[i]))
    s.close(); t.close()


# ---- 4. parity with the oracle stepped along each path ------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_verify_tree_meets_the_oracle(gpu, streams, weights, name):
    st, w = streams[name], weights[name]
    c = st.cfg
    pos0 = {"toy_gqa_unshared": 7, "stories15M": SEG - 3, "long_gqa": 5 * SEG + 220}[name]
    r = 3
    toks, g = planted(st, np.random.default_rng(40), BUSH, BUSH_PATH, r, pos0)
    s = gpu.RunState(c)
    feed_history(s, w, st.toks, pos0, False)
    nxt, path, a = s.verify_tree(toks, BUSH, pos0, w)
    assert a == r and path.tolist() == BUSH_PATH[:r + 1]
    dep = depths(BUSH)
    worst = 0.0

    def visit(i):   # preorder: when node i is stepped, the oracle's rows pos0 .. pos0 + depth - 1 are its ancestors'
        nonlocal worst
        ref = st.logits[pos0] if i == 0 else st.m.transformer(int(toks[i]), pos0 + dep[i])
        z = s.verify_logits(i)
        worst = max(worst, float(np.abs(z - ref).max()))
        np.testing.assert_allclose(z, ref, rtol=LOGIT_RTOL, atol=LOGIT_ATOL, err_msg=f"{name} node {i}")
        assert int(nxt[i]) == np_argmax(z)
        for ch in range(len(BUSH)):
            if BUSH[ch] == i:
                visit(ch)
    visit(0)
    for d in range(1, r + 1):   # the accepted path once more, for its KV rows
        st.m.transformer(int(toks[BUSH_PATH[d]]), pos0 + d)
    kvd = c.dim // c.n_heads * c.n_kv_heads
    nfl = c.n_layers * c.seq_len * kvd
    sl = slice(pos0, pos0 + r + 1)
    for mine, which in zip(caches(s, c), ("key_cache", "value_cache")):
        ref = st.m.state(which, nfl).reshape(c.n_layers, c.seq_len, kvd)
        np.testing.assert_allclose(mine[:, sl], ref[:, sl], rtol=KV_TOL, atol=KV_TOL)
    for p in range(pos0 + 1, pos0 + max(dep) + 1):   # the oracle's rows behind pos0 back to the stream's
        st.m.transformer(int(st.toks[p]), p)
    print(f"verify_tree parity {name}: max |logit diff| {worst:.3e}")
    s.close()


# ---- 5. the loops ---------------------------------------------------------------------------------------------------------------------

PROMPT = [9, 400, 77, 2001, 15]
STEPS = 40


def second_branch_drafter(full, vocab, right=True):
    """two chains below the root: the first wrong at every node, the second the known continuation (right=False: wrong too)"""
    def wrong(x, by):
        return (np.asarray(x, np.int64) - 2 + by) % (vocab - 2) + 2

    def draft(hist, depth, budget):
        true = np.asarray(full[len(hist):len(hist) + depth], np.int64)
        d = min(len(true), budget // 2)
        if d == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        first, second = wrong(true[:d], 1), (true[:d] if right else wrong(true[:d], 2))
        tok = np.concatenate([first, second]).astype(np.int32)
        par = np.array(list(range(d)) + [0] + list(range(d + 1, 2 * d)), np.int32)
        return tok, par
    return draft


def test_speculate_tree_emits_what_the_chain_loops_emit(gpu, ck):
    cfg = ck.STORIES15M
    w = gpu.Weights(cfg, None, True, seed=15)

    def run(f, *a, **kw):
        s = gpu.RunState(cfg)
        toks, stats = f(s, w, PROMPT, STEPS, *a, **kw)
        lg, kv = bits(s.logits()).copy(), [bits(x[:, :len(toks)]).copy() for x in caches(s, cfg)]
        s.close()
        return toks, stats, lg, kv

    def same_state(x, y, toks, what):
        if 1 not in toks.tolist():   # (a BOS ends the run wherever it stands in a call)
            assert np.array_equal(x[2], y[2]), (what, "final logits")
        for m, t in zip(x[3], y[3]):
            assert np.array_equal(m, t), (what, "cache rows below the next position")

    base = run(gpu.speculate_greedy, 0)
    s = gpu.RunState(cfg)
    s.greedy_begin(PROMPT)
    plain = s.greedy_run(w, STEPS)
    s.close()
    assert base[0].tolist() == plain.tolist()
    assert run(gpu.speculate_greedy, 4)[0].tolist() == base[0].tolist()
    full = [1] + base[0].tolist()
    for what, drafter in (("lookup", None), ("second branch", second_branch_drafter(full, cfg.vocab_size)),
                          ("always wrong", second_branch_drafter(full, cfg.vocab_size, right=False))):
        got = run(gpu.speculate_tree, 4, 15, drafter)
        toks, stats = got[0], got[1]
        assert toks.tolist() == base[0].tolist(), what
        same_state(got, base, toks, what)
        assert stats["emitted"] == len(toks) - len(PROMPT) - 1 and stats["accepted"] <= stats["offered"]
        if what == "second branch" and 1 not in toks.tolist():
            assert stats["accepted"] > 0 and stats["calls"] < base[1]["calls"]   # the walk took the second branch
        if what == "always wrong":
            assert stats["accepted"] == 0 and stats["offered"] > 0
        print(f"speculate_tree {what}: {stats}")
    # sampled: the ids of speculate_sample for one coin stream
    coins = gpu.coin_stream(77, STEPS)
    sbase = run(gpu.speculate_sample, 0, 1.0, 0.9, coins)
    assert run(gpu.speculate_sample, 4, 1.0, 0.9, coins)[0].tolist() == sbase[0].tolist()
    sfull = [1] + sbase[0].tolist()
    for what, drafter in (("lookup", None), ("second branch", second_branch_drafter(sfull, cfg.vocab_size)),
                          ("always wrong", second_branch_drafter(sfull, cfg.vocab_size, right=False))):
        got = run(gpu.speculate_tree, 4, 15, drafter, temperature=1.0, top_p=0.9, coins=coins)
        assert got[0].tolist() == sbase[0].tolist(), ("sampled", what)
        same_state(got, sbase, got[0], ("sampled", what))
        if what == "second branch" and 1 not in got[0].tolist():
            assert got[1]["accepted"] > 0
        print(f"speculate_tree sampled {what}: {got[1]}")
    w.close()


# ---- 6. refusals change nothing -------------------------------------------------------------------------------------------------

def test_verify_tree_contract_violations_change_nothing(gpu, ck):
    c = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    c2 = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=16)
    odd = ck.Config(dim=64, hidden_dim=174, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    w, w2, w_odd = gpu.Weights(c, None, False, seed=4), gpu.Weights(c2, None, False, seed=4), gpu.Weights(odd, None, False, seed=4)
    s, s_odd = gpu.RunState(c), gpu.RunState(odd)
    comm = gpu.Comm(0, 2, None, 0, emulated=True)
    shard = gpu.RunState(c, comm)
    s.prefill(np.array([3, 4, 5], np.int32), 0, w)
    s.verify_tree([6, 7, 8, 9], [-1, 0, 0, 1], 3, w, 1.0, 0.9, [0.1, 0.2, 0.3])   # the scratch exists

    def snap():
        return [np.concatenate([x.ravel() for x in caches(s, c)] + [s.logits()]).view(np.uint32)] + \
               [bits(s.verify_logits(r)).copy() for r in range(4)]
    before = snap()
    L = gpu.lib()
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    cfg_2 = gpu.L2ZConfig(*[int(v) for v in c2.as_i32()])
    nxt, path, acc = (C.c_int32 * 32)(), (C.c_int32 * 32)(), C.c_int(0)
    NULL = "null"

    def i32(v):
        return None if v is NULL else np.array(v, np.int32).ctypes.data_as(i32p)

    def call(tokens=(1, 2, 3, 4), parent=(-1, 0, 0, 1), n=None, pos0=5, temperature=0.0, top_p=1.0, coins=None, cfg=s.cfg,
             state=s, weights=w, o=nxt, p=path, a=acc):
        n = (0 if tokens is NULL else len(tokens)) if n is None else n
        return L.l2z_verify_tree(i32(tokens), i32(parent), n, pos0, C.c_float(temperature), C.c_float(top_p),
                                 None if coins is None else np.array(coins, np.float32).ctypes.data_as(fp),
                                 C.byref(cfg) if cfg is not None else None, state.h if state is not None else None,
                                 weights.h if weights is not None else None, o, p, C.byref(a) if a is not None else None)

    INV, STA = gpu.ERR_INVALID, gpu.ERR_STATE
    cases = [
        (dict(tokens=NULL, n=4), INV, "null tokens"), (dict(parent=NULL), INV, "null parent"), (dict(cfg=None), INV, "null config"),
        (dict(state=None), INV, "null runstate"), (dict(weights=None), INV, "null weights"), (dict(o=None), INV, "null out_next"),
        (dict(p=None), INV, "null out_path"), (dict(a=None), INV, "null out_accepted"),
        (dict(n=0), INV, "n_nodes = 0"), (dict(tokens=list(range(1, 18)), parent=[-1] + [0] * 16), INV, "n_nodes = 17"),
        (dict(parent=(0, 0, 0, 1)), INV, "parent[0] = 0"), (dict(parent=(-1, 0, 2, 1)), INV, "parent[i] = i"),
        (dict(parent=(-1, 0, 3, 1)), INV, "parent[i] > i"), (dict(parent=(-1, -1, 0, 1)), INV, "a second root"),
        (dict(tokens=(1, 2, 2, 4)), INV, "siblings with one token"), (dict(tokens=(1, 2, 3, 4, 4), parent=(-1, 0, 0, 1, 1)), INV, "deeper siblings with one token"),
        (dict(state=shard), INV, "a shard"), (dict(cfg=cfg_2), INV, "another config"), (dict(weights=w2), INV, "weights of another config"),
        (dict(cfg=s_odd.cfg, state=s_odd, weights=w_odd), INV, "dims not multiples of 4"),
        (dict(temperature=float("nan"), coins=(0.1, 0.2, 0.3)), INV, "temperature nan"),
        (dict(temperature=float("inf"), coins=(0.1, 0.2, 0.3)), INV, "temperature inf"),
        (dict(temperature=-0.5, coins=(0.1, 0.2, 0.3)), INV, "temperature < 0"),
        (dict(top_p=1.5), INV, "top_p > 1"), (dict(temperature=1.0, top_p=-0.1, coins=(0.1, 0.2, 0.3)), INV, "top_p < 0"),
        (dict(temperature=1.0), INV, "coins NULL at a temperature > 0"),
        (dict(temperature=1.0, coins=(0.1, 0.2, 1.0)), INV, "coin of the deepest level = 1"),
        (dict(temperature=1.0, coins=(-0.1, 0.2, 0.3)), INV, "coin < 0"),
        (dict(pos0=-1), STA, "pos0 < 0"), (dict(pos0=29), STA, "pos0 + n_nodes > seq_len"), (dict(pos0=32), STA, "pos0 = seq_len"),
        (dict(tokens=(1, -1, 3, 4)), STA, "token < 0"), (dict(tokens=(1, 2, 3, 512)), STA, "token = vocab"),
    ]
    for kw, code, what in cases:
        assert call(**kw) == code, what
    for b0, b1 in zip(before, snap()):
        assert np.array_equal(b0, b1)
    # what the rules let through: the last rows (n_nodes counts, not the depth); cousins with one token; a coin outside
    # [0, 1) below the deepest level read, or at temperature 0
    assert call(pos0=28) == gpu.OK
    assert call(tokens=(1, 2, 3, 4, 4), parent=(-1, 0, 0, 1, 2)) == gpu.OK
    assert call(temperature=1.0, coins=(0.1, 0.2, 0.3, 7.0)) == gpu.OK
    assert call(temperature=0.0, coins=(7.0, 7.0, 7.0)) == gpu.OK
    for x in (s, s_odd, shard):
        x.close()
    comm.close()
    for x in (w, w2, w_odd):
        x.close()
