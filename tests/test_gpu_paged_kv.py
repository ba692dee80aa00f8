"""The paged KV cache on the GPU (include/llama2_hip_test.h l2z_kvpool): runstates that draw 64-position pages
from a pool, in the four entry points of the wide family and in l2z_runstate_fork.

THE BAR IS BITS everywhere: np.array_equal on uint32 views.  The reference is the same calls on contiguous runstates in the
same process -- a page changes where a block finds its rows and no summation order, so ids, accepted counts, logits and
every KV row below a sequence's next position must be identical."""
import numpy as np
import pytest

from test_gpu_prefill_batch import bits, caches
from test_gpu_wide_decode import SHAPES

pytestmark = pytest.mark.gpu

SEED = 23
PAGE = 64
# the flow's two prompt passes: from 0, then on across (or exactly up to, or exactly from) the first page edge
LENS1 = [1, 5, 33, 1, 64, 17, 2]
LENS2 = [63, 60, 31, 64, 1, 47, 62]   # next positions 64, 65, 64, 65, 65, 64, 64
# (shape, L2Z_PF_X3): small -- the general attention form, head size 48, seq_len 320 = 5 pages; hs64 -- flash<4>, grouped kv
# heads; streams-2048 -- flash<8>, the bf16 cores (by shape, and forced); kvmul6 -- the 4 + 2 parts of wide_attention,
# seq_len 160 = a last page of 32 rows
FLOW_SHAPES = [("small", 1), ("hs64", 1), ("streams-2048", 1), ("streams-2048", 2), ("kvmul6", 1)]

_worlds = {}


@pytest.fixture(scope="module")
def world(gpu, ck):
    """shape -> (config, weights), made once per module"""
    def get(shape):
        if shape not in _worlds:
            cfg = ck.Config(**SHAPES[shape])
            _worlds[shape] = (cfg, gpu.Weights(cfg, None, False, seed=SEED))
        return _worlds[shape]
    yield get
    for _, w in _worlds.values():
        w.close()
    _worlds.clear()


def code_of(gpu, fn):
    with pytest.raises(gpu.L2ZError) as e:
        fn()
    return e.value.code


def rows_below(s, cfg, n):
    """KV rows 0 .. n - 1 of every layer, keys then values"""
    return [bits(x[:, :n, :]) for x in caches(s, cfg)]


def same_rows(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def attached(s):
    p = s.pages()
    return p[p >= 0]


def fill_pages(gpu, cfg, w, pool, n_pos):
    """a paged runstate that holds ceil(n_pos / 64) pages: one prompt pass of n_pos tokens"""
    s = gpu.RunState(cfg, pool=pool)
    t = np.random.default_rng([SEED, 99, n_pos]).integers(2, cfg.vocab_size, n_pos).astype(np.int32)
    t[0] = 1
    gpu.prefill_batch([s], [t], 0, w)
    return s


def flow(gpu, cfg, w, make, salt=0, guesses=None, after_first_call=None):
    """two prefill_batch calls, three transformer_wide steps, a sampled wide_run of 4 steps, a verify_wide whose guesses
    are partly wrong.  guesses=None: they are worked out here (the greedy continuation on contiguous forks, then one guess
    per sequence made wrong) and returned for the other runs of the same flow."""
    n, V = len(LENS1), cfg.vocab_size
    rng = np.random.default_rng([SEED, salt])
    states = [make() for _ in range(n)]
    t1 = [rng.integers(2, V, m).astype(np.int32) for m in LENS1]
    for t in t1:
        t[0] = 1
    t2 = [rng.integers(2, V, m).astype(np.int32) for m in LENS2]
    r = {"states": states}
    gpu.prefill_batch(states, t1, 0, w)
    if after_first_call is not None:
        after_first_call()
    gpu.prefill_batch(states, t2, LENS1, w)
    pos = np.array(LENS1, np.int32) + np.array(LENS2, np.int32)
    r["prompt_logits"] = [bits(s.logits()) for s in states]
    tok = gpu.argmax_batch(states)
    r["ids3"] = gpu.generate_wide(states, tok, pos, w, 3)
    pos = pos + 3
    coins = rng.random((4, n), dtype=np.float32)
    r["ids4"] = gpu.wide_run(states, r["ids3"][-1], pos, w, 4, temperature=1.0, top_p=0.9, coins=coins)
    pos = pos + 4
    last = r["ids4"][-1]
    if guesses is None:
        tmp = [gpu.RunState(cfg) for _ in range(n)]
        for t, s, p in zip(tmp, states, pos):
            gpu.runstate_fork(t, s, int(p))
        g = gpu.generate_wide(tmp, last, pos, w, 3)
        for t in tmp:
            t.close()
        guesses = []
        for j in range(n):
            gj = g[:2, j].copy().tolist() + [int(g[2, j])]
            if j % 4 < 3:
                gj[j % 4] = (gj[j % 4] + 1) % V   # sequence j's guess j % 4 is wrong (every fourth: none)
            guesses.append(np.array(gj, np.int32))
    r["guesses"] = guesses
    lists = [np.concatenate([[last[j]], guesses[j]]).astype(np.int32) for j in range(n)]
    nxt, acc = gpu.verify_wide(states, lists, pos, w)
    r["next"], r["accepted"] = np.concatenate(nxt), acc
    r["next_pos"] = pos + acc + 1
    r["logits"] = [bits(s.logits()) for s in states]
    r["rows"] = [rows_below(s, cfg, int(p)) for s, p in zip(states, r["next_pos"])]
    assert all(np.isfinite(s.logits()).all() for s in states)
    return r


def assert_same_flow(a, b):
    for k in ("ids3", "ids4", "next", "accepted", "next_pos"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("prompt_logits", "logits"):
        for j, (x, y) in enumerate(zip(a[k], b[k])):
            assert np.array_equal(x, y), (k, j)
    for j, (x, y) in enumerate(zip(a["rows"], b["rows"])):
        assert same_rows(x, y), ("KV rows", j)


def close_all(states):
    for s in states:
        s.close()


@pytest.mark.parametrize("shape,x3", FLOW_SHAPES, ids=[f"{s}-x3_{x}" for s, x in FLOW_SHAPES])
def test_identity_through_a_whole_flow(gpu, world, options, shape, x3):
    cfg, w = world(shape)
    options(L2Z_PF_X3=x3)
    ref = flow(gpu, cfg, w, lambda: gpu.RunState(cfg))
    assert len(set(ref["accepted"].tolist())) > 1, "the guesses are partly wrong: the accepted counts differ"
    pool = gpu.KvPool(cfg, 28)
    # a dummy of two pages, made and freed before the flow: the free list is no longer in ascending order ...
    fill_pages(gpu, cfg, w, pool, PAGE + 1).close()
    # ... and a second one that lives through the flow's first call, so that the two lowest pages go out as SECOND pages
    hole = fill_pages(gpu, cfg, w, pool, PAGE + 1)
    got = flow(gpu, cfg, w, lambda: gpu.RunState(cfg, pool=pool), guesses=ref["guesses"], after_first_call=hole.close)
    lists = [attached(s) for s in got["states"]]
    assert any(len(a) >= 2 and a[1] < a[0] and a[0] - a[1] > 1 for a in lists), lists   # neither ascending nor adjacent
    # a sequence holds the pages of every position it wrote: the verify call's four rows, accepted or not
    written = got["next_pos"] - got["accepted"] + 3
    assert [len(a) for a in lists] == [(int(e) + PAGE - 1) // PAGE for e in written], lists
    assert_same_flow(ref, got)
    used = sum(len(a) for a in lists)
    assert pool.info()["n_free"] == 28 - used
    close_all(ref["states"] + got["states"])
    assert pool.info()["n_free"] == 28
    pool.close()


@pytest.mark.parametrize("shape", ["small", "kvmul6"])
def test_page_edges(gpu, world, shape):
    """one transformer_wide step with rows at both sides of every page edge, on sequences forked from a prefilled
    contiguous base (the contiguous -> paged fork)"""
    cfg, w = world(shape)
    L = cfg.seq_len
    rng = np.random.default_rng([SEED, 2])
    prefix = np.array([1] + rng.integers(2, cfg.vocab_size, L - 2).tolist(), np.int32)
    base = gpu.RunState(cfg)
    base.prefill(prefix, 0, w)
    pos = np.array([0, 63, 64, 65, 127, 128, L - 1], np.int32)
    tok = rng.integers(2, cfg.vocab_size, len(pos)).astype(np.int32)
    tok[0] = 1
    need = sum((int(p) + PAGE) // PAGE for p in pos)
    pool = gpu.KvPool(cfg, need)
    ref = [gpu.RunState(cfg) for _ in pos]
    got = [gpu.RunState(cfg, pool=pool) for _ in pos]
    for ss in (ref, got):
        for s, p in zip(ss, pos):
            gpu.runstate_fork(s, base, int(p))
    # the fork attached ceil(p / 64) pages and copied the rows in
    assert [len(attached(s)) for s in got] == [(int(p) + PAGE - 1) // PAGE for p in pos]
    for a, b, p in zip(ref, got, pos):
        assert same_rows(rows_below(a, cfg, int(p)), rows_below(b, cfg, int(p)))
        assert np.array_equal(bits(a.logits()), bits(b.logits()))
    n_ref = gpu.transformer_wide(ref, tok, pos, w)
    n_got = gpu.transformer_wide(got, tok, pos, w)
    assert np.array_equal(n_ref, n_got)
    assert pool.info()["n_free"] == 0
    for a, b, p in zip(ref, got, pos):
        assert np.array_equal(bits(a.logits()), bits(b.logits())), p
        assert same_rows(rows_below(a, cfg, int(p) + 1), rows_below(b, cfg, int(p) + 1)), p
        # positions no page is attached for read as 0
        k = caches(b, cfg)[0]
        assert not k[:, len(attached(b)) * PAGE:, :].any()
    close_all(ref + got + [base])
    pool.close()


@pytest.mark.parametrize("shape", ["small", "hs64"])
def test_recycled_pages(gpu, world, shape):
    """flow B on the pages flow A gave back equals flow B on a fresh pool; a runstate that takes no part keeps its bits"""
    cfg, w = world(shape)
    pool = gpu.KvPool(cfg, 24)
    by = fill_pages(gpu, cfg, w, pool, 70)
    by_pages, by_rows, by_logits = by.pages(), rows_below(by, cfg, cfg.seq_len), bits(by.logits())
    a = flow(gpu, cfg, w, lambda: gpu.RunState(cfg, pool=pool), salt=1)
    close_all(a["states"])
    assert pool.info()["n_free"] == 24 - 2
    b1 = flow(gpu, cfg, w, lambda: gpu.RunState(cfg, pool=pool), salt=2)
    assert any(np.any(np.diff(attached(s)) < 0) for s in b1["states"])   # recycled: not in ascending order
    fresh = gpu.KvPool(cfg, 24)
    b2 = flow(gpu, cfg, w, lambda: gpu.RunState(cfg, pool=fresh), salt=2, guesses=b1["guesses"])
    assert_same_flow(b2, b1)
    assert np.array_equal(by.pages(), by_pages)
    assert same_rows(rows_below(by, cfg, cfg.seq_len), by_rows) and np.array_equal(bits(by.logits()), by_logits)
    close_all(b1["states"] + b2["states"] + [by])
    pool.close()
    fresh.close()


def test_exhaustion(gpu, world):
    cfg, w = world("small")
    n, V = 3, cfg.vocab_size
    rng = np.random.default_rng([SEED, 4])
    prompts = [np.array([1] + rng.integers(2, V, 59).tolist(), np.int32) for _ in range(n)]
    pool = gpu.KvPool(cfg, 5)
    ref = [gpu.RunState(cfg) for _ in range(n)]
    got = [gpu.RunState(cfg, pool=pool) for _ in range(n)]
    toks = {}
    for name, ss in (("ref", ref), ("got", got)):
        gpu.prefill_batch(ss, prompts, 0, w)
        toks[name] = gpu.generate_wide(ss, gpu.argmax_batch(ss), 60, w, 4)   # positions 60 .. 63: still page 0
    assert np.array_equal(toks["ref"], toks["got"])
    tok = toks["ref"][-1]
    # the step that crosses the edge needs 3 pages, 2 are free
    def snap():
        return pool.info()["n_free"], [s.pages().tolist() for s in got], [bits(s.logits()) for s in got]
    before = snap()
    assert before[0] == 2
    assert code_of(gpu, lambda: gpu.transformer_wide(got, tok, [64] * n, w)) == gpu.ERR_OOM
    assert code_of(gpu, lambda: gpu.wide_run(got, tok, [63] * n, w, 2)) == gpu.ERR_OOM   # its SECOND step crosses
    after = snap()
    assert after[0] == before[0] and after[1] == before[1]
    assert all(np.array_equal(x, y) for x, y in zip(before[2], after[2]))
    got[2].trim(0)
    assert pool.info()["n_free"] == 3 and len(attached(got[2])) == 0
    # a sequence whose lower pages are gone is refused, never read through
    assert code_of(gpu, lambda: gpu.transformer_wide(got, tok, [64] * n, w)) == gpu.ERR_STATE
    got[2].close()
    n_ref = gpu.transformer_wide(ref[:2], tok[:2], [64, 64], w)
    n_got = gpu.transformer_wide(got[:2], tok[:2], [64, 64], w)
    assert np.array_equal(n_ref, n_got) and pool.info()["n_free"] == 1
    for a, b in zip(ref[:2], got[:2]):
        assert np.array_equal(bits(a.logits()), bits(b.logits()))
        assert same_rows(rows_below(a, cfg, 65), rows_below(b, cfg, 65))
    close_all(ref + got[:2])
    pool.close()


def test_shared_prefix(gpu, world):
    cfg, w = world("small")
    V, n_forks, n_pos = cfg.vocab_size, 8, 130
    rng = np.random.default_rng([SEED, 5])
    prompt = np.array([1] + rng.integers(2, V, 199).tolist(), np.int32)
    pool = gpu.KvPool(cfg, 16)
    sides = {}
    for name, make in (("ref", lambda: gpu.RunState(cfg)), ("got", lambda: gpu.RunState(cfg, pool=pool))):
        base = make()
        gpu.prefill_batch([base], [prompt], 0, w)
        if name == "got":
            assert pool.info()["n_free"] == 16 - 4
        forks = [make() for _ in range(n_forks)]
        for f in forks:
            gpu.runstate_fork(f, base, n_pos)
        sides[name] = (base, forks)
    base, forks = sides["got"]
    # 2 whole pages shared by all nine, one private page per fork for rows 128, 129: 8 pages more, not 24
    assert pool.info()["n_free"] == 16 - 4 - n_forks
    for f in forks:
        assert np.array_equal(f.pages()[:2], base.pages()[:2]) and f.pages()[2] not in base.pages()
    assert len({int(f.pages()[2]) for f in forks}) == n_forks
    tok = rng.integers(2, V, n_forks).astype(np.int32)
    ids = {name: gpu.generate_wide(sides[name][1], tok, n_pos, w, 3) for name in ("ref", "got")}
    assert np.array_equal(ids["ref"], ids["got"])
    for a, b in zip(sides["ref"][1], forks):
        assert np.array_equal(bits(a.logits()), bits(b.logits()))
        assert same_rows(rows_below(a, cfg, n_pos + 3), rows_below(b, cfg, n_pos + 3))
    # the base steps on unaffected: position 200 lies in its own fourth page
    nb = {name: gpu.transformer_wide([sides[name][0]], [7], [200], w) for name in ("ref", "got")}
    assert np.array_equal(nb["ref"], nb["got"])
    assert np.array_equal(bits(sides["ref"][0].logits()), bits(base.logits()))
    assert same_rows(rows_below(sides["ref"][0], cfg, 201), rows_below(base, cfg, 201))
    # ... but may not write below the fork point any more, and neither may a fork
    free = pool.info()["n_free"]
    snap = [f.pages().tolist() for f in forks], bits(forks[0].logits())
    assert code_of(gpu, lambda: gpu.transformer_wide([base], [7], [100], w)) == gpu.ERR_STATE
    # closing the base leaves the forks' rows intact and frees its two private pages only
    rows0 = rows_below(forks[0], cfg, n_pos + 3)
    base.close()
    assert pool.info()["n_free"] == free + 2
    assert same_rows(rows_below(forks[0], cfg, n_pos + 3), rows0)
    assert code_of(gpu, lambda: gpu.transformer_wide([forks[0]], [7], [100], w)) == gpu.ERR_STATE
    assert code_of(gpu, lambda: gpu.verify_wide([forks[0]], [[7, 8, 9]], [126], w)) == gpu.ERR_STATE   # 126, 127: shared
    assert pool.info()["n_free"] == free + 2
    assert [f.pages().tolist() for f in forks] == snap[0] and np.array_equal(bits(forks[0].logits()), snap[1])
    assert same_rows(rows_below(forks[0], cfg, n_pos + 3), rows0)
    # when every other holder has let go, the last one may write again
    close_all(forks[1:])
    gpu.transformer_wide([forks[0]], [7], [100], w)
    close_all([forks[0], sides["ref"][0]] + sides["ref"][1])
    assert pool.info()["n_free"] == 16
    pool.close()


def test_refusals(gpu, ck):
    cfg = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=96)
    other = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=128)
    w = gpu.Weights(cfg, None, False, seed=4)
    pool, pool2 = gpu.KvPool(cfg, 4), gpu.KvPool(cfg, 4)
    s, s2, c = gpu.RunState(cfg, pool=pool), gpu.RunState(cfg, pool=pool2), gpu.RunState(cfg)
    t = np.array([1, 5, 7], np.int32)
    half = np.array([0.5, 0.5, 0.5], np.float32)
    calls = {
        "l2z_transformer": lambda: s.transformer(1, 0, w),
        "l2z_prefill": lambda: s.prefill(t, 0, w),
        "l2z_score": lambda: s.score(t, 0, w),
        "l2z_greedy_begin": lambda: s.greedy_begin([1, 2]),
        "l2z_greedy_run": lambda: s.greedy_run(w, 2),
        "l2z_sample_run": lambda: s.sample_run(w, 2, 1.0, 0.9, half),
        "l2z_transformer_batch": lambda: gpu.transformer_batch([s], [1], [0], w),
        "l2z_batch_time": lambda: gpu.batch_time([s], [1], [0], w, 1),
        "l2z_verify": lambda: s.verify(t, 0, w),
        "l2z_verify_time": lambda: s.verify_time(t, 0, w, 1),
        "l2z_verify_sample": lambda: s.verify_sample(t, 0, w, 1.0, 0.9, half),
        "l2z_verify_sample_time": lambda: s.verify_sample_time(t, 0, w, 1.0, 0.9, half, 1),
        "l2z_verify_batch": lambda: gpu.verify_batch([s], [t], [0], w),
        "l2z_verify_tree": lambda: s.verify_tree(t, [-1, 0, 0], 0, w),
        "l2z_verify_tree_time": lambda: s.verify_tree_time(t, [-1, 0, 0], 0, w, 1),
        "l2z_profile_forward": lambda: s.profile_forward(1, 0, w),
        "l2z_time_kind": lambda: s.time_kind("qkv", 0, w),
        "l2z_emu_transformer": lambda: gpu.emu_transformer([s], [w], 1, 0),
        "l2z_emu_prefill": lambda: gpu.emu_prefill([s], [w], t, 0),
    }
    for name, fn in calls.items():
        assert code_of(gpu, fn) == gpu.ERR_INVALID, name
    assert pool.info()["n_free"] == 4 and len(attached(s)) == 0
    # one kind per call, one pool per call, the pool's own config
    one = np.array([1], np.int32)
    assert code_of(gpu, lambda: gpu.transformer_wide([s, c], [1, 1], [0, 0], w)) == gpu.ERR_INVALID
    assert code_of(gpu, lambda: gpu.transformer_wide([c, s], [1, 1], [0, 0], w)) == gpu.ERR_INVALID
    assert code_of(gpu, lambda: gpu.prefill_batch([s, c], [one, one], 0, w)) == gpu.ERR_INVALID
    assert code_of(gpu, lambda: gpu.wide_run([s, c], [1, 1], [0, 0], w, 2)) == gpu.ERR_INVALID
    assert code_of(gpu, lambda: gpu.verify_wide([s, c], [one, one], [0, 0], w)) == gpu.ERR_INVALID
    assert code_of(gpu, lambda: gpu.transformer_wide([s, s2], [1, 1], [0, 0], w)) == gpu.ERR_INVALID
    assert code_of(gpu, lambda: gpu.RunState(other, pool=pool)) == gpu.ERR_INVALID
    assert code_of(gpu, pool.close) == gpu.ERR_STATE   # a runstate made from it is alive
    assert pool.info() == {"n_pages": 4, "n_free": 4, "page_bytes": 2 * 2 * 2 * PAGE * 16 * 4}
    assert pool2.info()["n_free"] == 4 and len(attached(s2)) == 0
    # ... and the runstate is as usable as before: the wide family and the logits-only calls
    gpu.prefill_batch([s], [t], 0, w)
    gpu.prefill_batch([c], [t], 0, w)
    assert np.array_equal(bits(s.logits()), bits(c.logits()))
    assert s.argmax() == c.argmax() and np.array_equal(gpu.argmax_batch([s, c]), gpu.argmax_batch([c, s])[::-1])
    assert np.array_equal(gpu.sample_batch([s, c], 1.0, 0.9, 0.25), gpu.sample_batch([c, s], 1.0, 0.9, 0.25)[::-1])
    assert np.array_equal(bits(s.probs(1.0)), bits(c.probs(1.0)))
    s.synchronize()
    for x in (s, s2, c):
        x.close()
    pool.close()
    pool2.close()
    w.close()
