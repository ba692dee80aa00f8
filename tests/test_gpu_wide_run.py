"""l2z_wide_run on the GPU: n_steps wide decode steps of up to 128 sequences in one call, every row's token drawn on the
device (wide_sample.hip) and handed to the next step there.

THE DEFINING PROPERTY is checked bit for bit: the ids, every row's final logits and the WHOLE key and value caches of
every runstate equal those of the step loop on runstates forked from the same prefix at the same depths -- the loop of
l2z_transformer_wide(out_next = NULL) and l2z_sample_batch in groups of 16, built from entry points that stood before the
run did.  The values themselves are the step's and the sampler's, pinned against the CPU oracle and the host samplers in
tests/test_gpu_wide_decode.py and tests/test_gpu_sample_batch.py; nothing here has a tolerance.

Every runstate starts as a fork of ONE prefilled prefix at its own depth over a cache full of another sequence's rows, so
that every row beyond a runstate's depth holds a stale pattern.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_prefill_batch import SHAPES, bits, caches
from test_gpu_wide_decode import SEED, forked

pytestmark = pytest.mark.gpu

STEPS = 6
ALMOST_ONE = np.nextafter(np.float32(1.0), np.float32(0.0))   # the largest float32 below 1
# (temperature, top_p, coins: None = drawn from the seeded generator) -- row i takes SETTINGS[i % 7]
SETTINGS = [(1.0, 0.9, None),          # the reference's default: sample_top_p
            (1.0, 1.0, None),          # the plain `sample` path ...
            (0.7, 0.0, None),          # ... from either end of top_p
            (0.05, 0.9, None),         # peaked: few candidates
            (1.0, 0.9, 0.0),           # coins all 0
            (1.0, 0.9, ALMOST_ONE),    # coins at the largest float32 below 1
            (0.0, 0.9, None)]          # temperature 0: the argmax, the coin is not read


class World:
    """a shape on the GPU: its weights, a prefix in a base runstate, and a runstate whose every cache row is stale"""

    def __init__(self, gpu, ck, shape):
        self.gpu = gpu
        self.cfg = ck.Config(**SHAPES[shape])
        L = self.cfg.seq_len
        rng = np.random.default_rng([SEED[shape], 11])
        self.w = gpu.Weights(self.cfg, ck.synth_blob(self.cfg, False, seed=SEED[shape]), False)
        self.base, self.garbage = gpu.RunState(self.cfg), gpu.RunState(self.cfg)
        self.base.prefill(np.array([1] + rng.integers(2, self.cfg.vocab_size, L - 2).tolist(), np.int32), 0, self.w)
        self.garbage.prefill(rng.integers(2, self.cfg.vocab_size, L).astype(np.int32), 0, self.w)

    def fork(self, depths, base=None):
        return [forked(self.gpu, base or self.base, int(p), self.garbage) for p in depths]

    def close(self):
        self.base.close()
        self.garbage.close()
        self.w.close()


@pytest.fixture(scope="module")
def worlds(gpu, ck):
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = World(gpu, ck, shape)
        return made[shape]
    yield get
    for wd in made.values():
        wd.close()


def plan(cfg, n, steps=STEPS, salt=0, room=0):
    """n rows: depths (a row crossing the segment edge at 64 first -- 61 .. 66, so the grid's extent grows mid-run --, a
    row from 0, a row ending on the last position, a row crossing 125 .. 130, then seeded ones), first tokens, and the
    rows' settings as arrays.  room: positions left free behind every row's last step (for what goes on afterwards)"""
    L, V = cfg.seq_len, cfg.vocab_size
    rng = np.random.default_rng([5, n, salt])
    last = L - steps - room
    edges = [p for p in (61, 0, last, 125) if p <= last]
    pos = np.array((edges + rng.integers(0, last + 1, n).tolist())[:n], np.int32)
    tok = rng.integers(2, V, n).astype(np.int32)
    tok[pos == 0] = 1
    temp = np.array([SETTINGS[i % 7][0] for i in range(n)], np.float32)
    topp = np.array([SETTINGS[i % 7][1] for i in range(n)], np.float32)
    coins = rng.random((steps, n), np.float32)
    for i in range(n):
        if SETTINGS[i % 7][2] is not None:
            coins[:, i] = SETTINGS[i % 7][2]
    assert coins.min() >= 0.0 and coins.max() < 1.0
    return pos, tok, temp, topp, coins


def step_loop(gpu, states, tok, pos, w, temp, topp, coins):
    """the loop the run replaces, from entry points that stood before it: a wide step, then the draws in groups of 16"""
    n, ids = len(states), []
    tok = np.array(tok, np.int32)
    for k in range(coins.shape[0]):
        gpu.transformer_wide(states, tok, pos + k, w, want_next=False)
        tok = np.concatenate([gpu.sample_batch(states[g:g + 16], temp[g:g + 16], topp[g:g + 16], coins[k, g:g + 16])
                              for g in range(0, n, 16)]).astype(np.int32)
        ids.append(tok)
    return np.stack(ids)


def snap(states, cfg):
    """(logits, key cache, value cache) of every runstate, as bits"""
    return [(bits(s.logits()),) + tuple(bits(x) for x in caches(s, cfg)) for s in states]


def assert_same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        for name, p, q in zip(("logits", "key cache", "value cache"), x, y):
            assert np.array_equal(p, q), (what, "row", i, name)


def close(*groups):
    for g in groups:
        for s in g:
            s.close()


CASES = [("small", n) for n in (1, 16, 17, 33, 128)] + [("hs64", 33), ("streams-2048", 33)]


@pytest.mark.parametrize("shape,n", CASES, ids=[f"{s}-{n}" for s, n in CASES])
def test_run_equals_the_step_loop_bit_for_bit(gpu, ck, worlds, shape, n):
    wd = worlds(shape)
    pos, tok, temp, topp, coins = plan(wd.cfg, n)
    if n >= 4:
        want = {61, 0, wd.cfg.seq_len - STEPS} | ({125} if wd.cfg.seq_len >= 131 + STEPS else set())
        assert want <= set(pos.tolist())
    if n >= 7:
        assert len(set(zip(temp.tolist(), topp.tolist()))) == 5 and 0.0 in temp   # every kind of row is in the batch
    run, loop = wd.fork(pos), wd.fork(pos)
    ids = gpu.wide_run(run, tok, pos, wd.w, STEPS, temp, topp, coins)
    ref = step_loop(gpu, loop, tok, pos, wd.w, temp, topp, coins)
    assert ids.shape == (STEPS, n) and ids.dtype == np.int32
    assert np.array_equal(ids, ref), (shape, n, np.argwhere(ids != ref)[:4].tolist())
    assert_same(snap(run, wd.cfg), snap(loop, wd.cfg), (shape, n))
    close(run, loop)


def test_all_greedy_equals_generate_wide(gpu, ck, worlds):
    wd = worlds("small")
    n = 33
    pos, tok, _, _, _ = plan(wd.cfg, n, salt=1)
    run, loop = wd.fork(pos), wd.fork(pos)
    ids = gpu.wide_run(run, tok, pos, wd.w, STEPS)
    ref = gpu.generate_wide(loop, tok, pos, wd.w, STEPS)
    assert np.array_equal(ids, ref)
    assert_same(snap(run, wd.cfg), snap(loop, wd.cfg), "greedy")
    # ... and temperature 0 on every row is the same run
    zero = wd.fork(pos)
    assert np.array_equal(gpu.wide_run(zero, tok, pos, wd.w, STEPS, 0.0, 0.9, None), ref)
    assert_same(snap(zero, wd.cfg), snap(loop, wd.cfg), "temperature 0")
    close(run, loop, zero)


def test_footprint_only_the_steps_rows_of_the_calls_runstates(gpu, ck, worlds):
    wd = worlds("small")
    cfg, n = wd.cfg, 33
    pos, tok, temp, topp, coins = plan(cfg, n, salt=2)
    run = wd.fork(pos)
    absent = wd.fork([0, 61, cfg.seq_len - STEPS])
    before, before_absent = snap(run, cfg), snap(absent, cfg)
    gpu.wide_run(run, tok, pos, wd.w, STEPS, temp, topp, coins)
    after = snap(run, cfg)
    for i in range(n):
        keep = np.ones(cfg.seq_len, bool)
        keep[pos[i]:pos[i] + STEPS] = False
        for name, was, got in zip(("key", "value"), before[i][1:], after[i][1:]):
            assert np.array_equal(got[:, keep], was[:, keep]), (i, name, "a row outside the steps' changed")
            assert not np.array_equal(got[:, ~keep], was[:, ~keep]), (i, name, "the steps' rows were not written")
    assert_same(snap(absent, cfg), before_absent, "runstates absent from the call")
    close(run, absent)


def test_every_entry_point_goes_on_from_the_run(gpu, ck, worlds):
    """after the run, and after the step loop on the twin set: l2z_argmax on a row, l2z_runstate_fork +
    l2z_transformer_batch on a group, l2z_transformer_wide on all rows -- the same bits"""
    wd = worlds("small")
    cfg, n = wd.cfg, 33
    pos, tok, temp, topp, coins = plan(cfg, n, salt=3, room=2)
    run, loop = wd.fork(pos), wd.fork(pos)
    ids = gpu.wide_run(run, tok, pos, wd.w, STEPS, temp, topp, coins)
    assert np.array_equal(ids, step_loop(gpu, loop, tok, pos, wd.w, temp, topp, coins))
    for i in (0, 1, n - 1):
        assert run[i].argmax() == loop[i].argmax() == int(np.argmax(run[i].logits()))
    then = pos + STEPS
    groups = []
    for src in (run, loop):
        g = [gpu.RunState(cfg) for _ in range(16)]
        for d, s, p in zip(g, src[:16], then[:16]):
            gpu.runstate_fork(d, s, int(p))
        gpu.transformer_batch(g, ids[-1, :16], then[:16], wd.w)
        groups.append(g)
    assert_same(snap(groups[0], cfg), snap(groups[1], cfg), "fork + batched step")
    a = gpu.transformer_wide(run, ids[-1], then, wd.w)
    b = gpu.transformer_wide(loop, ids[-1], then, wd.w)
    assert np.array_equal(a, b)
    assert_same(snap(run, cfg), snap(loop, cfg), "wide step")
    close(run, loop, *groups)


def test_neighbour_invariance_of_the_run(gpu, ck, worlds):
    """n = 33: the kept rows' ids, final logits and cache rows are the same bits when every other row's first token, depth,
    cache contents, temperature and coins change"""
    wd = worlds("small")
    cfg, n = wd.cfg, 33
    L = cfg.seq_len
    rng = np.random.default_rng([SEED["small"], 12])
    pos, tok, temp, topp, coins = plan(cfg, n, salt=4)

    def result(states, ids, p):
        out = []
        for i, s in enumerate(states):
            k, v = caches(s, cfg)
            out.append((ids[:, i].copy(), bits(s.logits()), bits(k[:, p[i]:p[i] + STEPS]), bits(v[:, p[i]:p[i] + STEPS])))
        return out

    first_states = wd.fork(pos)
    first = result(first_states, gpu.wide_run(first_states, tok, pos, wd.w, STEPS, temp, topp, coins), pos)
    other_base = gpu.RunState(cfg)
    other_base.prefill(np.array([1] + rng.integers(2, cfg.vocab_size, L - 2).tolist(), np.int32), 0, wd.w)
    for part in (0, 1):   # the rows kept in this run: every second one
        kept = np.arange(n) % 2 == part
        p2 = np.where(kept, pos, rng.integers(0, L - STEPS + 1, n)).astype(np.int32)
        if part == 0:
            p2[1] = L - STEPS   # a neighbour deeper than every kept row of this half: the grids' segment extent grows
        t2 = np.where(kept, tok, rng.integers(2, cfg.vocab_size, n)).astype(np.int32)
        te2 = np.where(kept, temp, np.roll(temp, 1)).astype(np.float32)
        tp2 = np.where(kept, topp, np.roll(topp, 1)).astype(np.float32)
        c2 = np.where(kept[None, :], coins, rng.random((STEPS, n), np.float32)).astype(np.float32)
        states = [forked(gpu, wd.base if kept[i] else other_base, int(p2[i]), wd.garbage) for i in range(n)]
        got = result(states, gpu.wide_run(states, t2, p2, wd.w, STEPS, te2, tp2, c2), p2)
        for i in np.flatnonzero(kept):
            for name, x, y in zip(("ids", "logits", "key rows", "value rows"), first[i], got[i]):
                assert np.array_equal(x, y), ("neighbours", part, int(i), name)
        close(states)
    close(first_states, [other_base])


def test_two_calls_of_three_steps_equal_one_call_of_six(gpu, ck, worlds):
    wd = worlds("small")
    n = 33
    pos, tok, temp, topp, coins = plan(wd.cfg, n, salt=5)
    one, two = wd.fork(pos), wd.fork(pos)
    ids = gpu.wide_run(one, tok, pos, wd.w, 6, temp, topp, coins)
    a = gpu.wide_run(two, tok, pos, wd.w, 3, temp, topp, coins[:3])
    b = gpu.wide_run(two, a[-1], pos + 3, wd.w, 3, temp, topp, coins[3:])
    assert np.array_equal(np.concatenate([a, b]), ids)
    assert_same(snap(one, wd.cfg), snap(two, wd.cfg), "3 + 3")
    close(one, two)


def test_generate_wide_sample_cuts_each_column_after_its_first_bos(gpu, ck, worlds):
    wd = worlds("small")
    n = 17
    pos, tok, temp, topp, coins = plan(wd.cfg, n, salt=6)
    a, b = wd.fork(pos), wd.fork(pos)
    ids = gpu.wide_run(a, tok, pos, wd.w, STEPS, temp, topp, coins)
    bos = int(ids[2, 3])   # (a synthetic model draws the real BOS too rarely to meet it: any id serves as the mark)
    cols = gpu.generate_wide_sample(b, tok, pos, wd.w, STEPS, temp, topp, coins, bos=bos)
    assert len(cols) == n
    for i, col in enumerate(cols):
        hit = np.flatnonzero(ids[:, i] == bos)
        want = ids[:hit[0] + 1, i] if hit.size else ids[:, i]
        assert np.array_equal(col, want), i
    assert len(cols[3]) <= 3
    close(a, b)


def test_contract_refusals_change_nothing(gpu, ck):
    c = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    w = gpu.Weights(c, None, False, seed=4)
    ss = [gpu.RunState(c) for _ in range(gpu.WIDE_MAX + 1)]
    for i, s in enumerate(ss[:3]):
        s.prefill(np.array([3 + i, 4, 5], np.int32), 0, w)

    def snap3():
        return [(np.concatenate([bits(x).ravel() for x in caches(s, c)]), bits(s.logits())) for s in ss[:3]]
    before = snap3()
    L = gpu.lib()
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    nan, inf = float("nan"), float("inf")

    def call(states, toks, pos, steps=2, temp=None, topp=None, coins=None, n=None, null=()):
        n = len(states) if n is None else n
        arr = (C.c_void_p * max(len(states), 1))(*[s.h for s in states])
        t, p = np.array(toks, np.int32), np.array(pos, np.int32)
        fl = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (temp, topp, coins)]
        out = np.zeros(max(steps, 1) * max(len(states), 1), np.int32)
        args = [n, t.ctypes.data_as(i32), p.ctypes.data_as(i32), steps] + \
               [None if v is None else v.ctypes.data_as(f32) for v in fl] + \
               [C.byref(ss[0].cfg), arr, w.h, out.ctypes.data_as(i32)]
        for k in null:
            args[k] = C.cast(None, i32) if k in (1, 2, 10) else None
        return L.l2z_wide_run(*args)

    a, b = ss[0], ss[1]
    ok = dict(temp=[1.0, 0.0], topp=[0.9, 0.9], coins=[[0.5, 0.5], [0.25, 0.5]])
    INV, ST = gpu.ERR_INVALID, gpu.ERR_STATE
    # everything l2z_transformer_wide refuses
    assert call([a], [1], [3], n=0) == INV
    assert call(ss, [1] * len(ss), [3] * len(ss)) == INV                            # n = 129
    assert call([a, b, a], [1, 1, 1], [3, 3, 3]) == INV                             # the same runstate twice
    for k in (1, 2, 7, 8, 9, 10):                                                   # tokens, pos0, config, states, w, out
        assert call([a, b], [1, 1], [3, 3], null=(k,), **ok) == INV, k
    assert call([a, b], [1, 1], [3, 3], steps=0, **ok) == INV
    assert call([a, b], [1, 1], [3, 3], steps=-1, **ok) == INV
    # the sampler's rules
    for bad in (nan, inf, -1.0):
        assert call([a, b], [1, 1], [3, 3], **dict(ok, temp=[1.0, bad])) == INV, bad
    for bad in (-0.1, 1.5, nan):
        assert call([a, b], [1, 1], [3, 3], **dict(ok, topp=[0.9, bad])) == INV, bad   # (a greedy row's too, as l2z_sample_batch)
    assert call([a, b], [1, 1], [3, 3], **dict(ok, topp=None)) == INV
    assert call([a, b], [1, 1], [3, 3], **dict(ok, coins=None)) == INV
    for bad in (1.0, -0.1, nan):
        assert call([a, b], [1, 1], [3, 3], **dict(ok, coins=[[0.5, 0.5], [bad, 0.5]])) == INV, bad   # the LAST step's coin
    # positions and tokens
    assert call([a, b], [1, 1], [-1, 3], **ok) == ST
    assert call([a, b], [1, 1], [3, c.seq_len - 1], **ok) == ST                     # 31 + 2 steps > seq_len
    assert call([a, b], [1, 1], [3, c.seq_len], **ok) == ST
    assert call([a, b], [1, c.vocab_size], [3, 3], **ok) == ST
    assert call([a, b], [-1, 1], [3, 3]) == ST
    for (k0, l0), (k1, l1) in zip(before, snap3()):
        assert np.array_equal(k0, k1) and np.array_equal(l0, l1)
    # the bookkeeping is as before: a wide step at the old position still succeeds ...
    gpu.transformer_wide([a, b], [1, 1], [3, 3], w)
    # ... and the same arguments are accepted once they are right: a greedy row's coin is not read, the last position is
    # reachable, all greedy needs no sampler argument, 128 runstates
    assert call([a, b], [1, 1], [3, c.seq_len - 2], **dict(ok, coins=[[0.5, nan], [0.25, 7.0]])) == gpu.OK
    assert not np.array_equal(bits(a.logits()), before[0][1])
    assert call([a, b], [1, 1], [3, 3]) == gpu.OK
    assert call([a, b], [1, 1], [3, 3], temp=[0.0, 0.0], topp=[1.0, 1.0]) == gpu.OK   # (no coins: no row draws)
    assert call(ss[:gpu.WIDE_MAX], [1] * gpu.WIDE_MAX, [0] * gpu.WIDE_MAX, temp=[0.5] * gpu.WIDE_MAX, topp=[0.9] * gpu.WIDE_MAX,
                coins=np.full((2, gpu.WIDE_MAX), 0.5)) == gpu.OK
    for s in ss:
        s.close()
    w.close()
