"""l2z_verify_wide on the GPU: the verify pass for up to 128 rows of many sequences, up to 16 consecutive positions each, as
one chunk of the ragged prompt pass with the multi-row segment attention and the verdict of wide_verify.hip.

What the header promises is checked as it is stated: ONE-ROW IDENTITY with l2z_transformer_wide, NEIGHBOUR INVARIANCE,
CAUSALITY, THE DRAW and the cache footprint bit for bit (np.array_equal on whole caches and logits); PARITY against
l2z_verify on a forked twin of each sequence alone within twice THE BAR of tests/test_gpu_parity.py (LOGIT_ATOL +
LOGIT_RTOL * max |z|) and KV rows within 2e-5 -- the margins tests/test_gpu_wide_decode.py uses between two GPU forms --
and, on `small` at 33 rows, against the CPU oracle at the bar itself.

Every runstate starts as a fork of ONE prefilled prefix at its own depth over a cache full of another sequence's rows, so
that every row beyond a runstate's depth holds a stale pattern (tests/test_gpu_wide_run.py's set-up).

The layouts.  The row counts 1, 2, 3, 4, 5, 8, 9 and 16 add up to 48, so a layout of 17 or 33 rows cannot hold them all:
the 128-row layout holds every one (9 there alone), and the smaller ones hold the others between them (17: 8, 1, 2, 6;
33a: 1, 8, 2, 6, 3, 4, 5, 4; 33b: 16, 8, 1, 2, 6), so that every instantiation of the attention (1, 2, 4, 8, 16 slots) runs
full and partly used.  EVERY layout holds a sequence from position 0, one of 8 rows from 60 (its rows 0 .. 3 end before
segment 1: the i0 mask, at 17 rows on the short-prompt products too), one from 64 and one crossing 125 .. 130; the 33- and
128-row layouts one ending on seq_len - 1 as well, for which 17 rows have no room.  Sequence j draws with SETTINGS[j % 7]: a
greedy sequence beside (1.0, 0.9), (1.0, 1.0), (0.7, 0.0), the peaked (0.05, 0.9), coins of 0 and of the largest float32
below 1.

Not constructible on a machine with one GPU, and so not called here: runstates on two devices.  A runstate's next position
(the host's bookkeeping) cannot be read back through the binding and no entry point refuses a position because of it, so
"a refusal leaves the next positions unchanged" is NOT observable here: the refusal test checks caches, logits and the
hook's matrix bit for bit, and that later calls are accepted.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import LOGIT_ATOL, LOGIT_RTOL
from test_gpu_prefill_batch import bits, caches
from test_gpu_wide_decode import SEED, SHAPES, forked
from test_gpu_wide_run import SETTINGS

pytestmark = pytest.mark.gpu

KV_TOL = 2e-5


def bar_of(z):
    return LOGIT_ATOL + LOGIT_RTOL * float(np.abs(z).max())


def layout(cfg, name):
    """[(pos0, rows)] of a named layout"""
    L = cfg.seq_len
    return {"17": [(60, 8), (0, 1), (64, 2), (125, 6)],
            "33a": [(0, 1), (60, 8), (64, 2), (125, 6), (L - 3, 3), (30, 4), (200, 5), (100, 4)],
            "33b": [(L - 16, 16), (60, 8), (0, 1), (64, 2), (125, 6)],
            "128": [(0, 1), (60, 8), (64, 2), (125, 9), (L - 3, 3), (30, 4), (200, 5), (150, 16), (10, 16), (70, 16),
                    (180, 16), (250, 16), (40, 9), (90, 5), (L - 2, 2)]}[name]


class World:
    """a shape on the GPU: its weights, a prefix in a base runstate, and a runstate whose every cache row is stale"""

    def __init__(self, gpu, ck, shape):
        self.gpu, self.shape = gpu, shape
        self.cfg = ck.Config(**SHAPES[shape])
        L = self.cfg.seq_len
        rng = np.random.default_rng([SEED[shape], 21])
        self.blob = ck.synth_blob(self.cfg, False, seed=SEED[shape])
        self.w = gpu.Weights(self.cfg, self.blob, False)
        self.prefix = np.array([1] + rng.integers(2, self.cfg.vocab_size, L - 2).tolist(), np.int32)
        self.base, self.garbage = gpu.RunState(self.cfg), gpu.RunState(self.cfg)
        self.base.prefill(self.prefix, 0, self.w)
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


class Case:
    """a layout on a shape: positions, row counts, tokens (a first token and random guesses), and every sequence's draw"""

    def __init__(self, cfg, name, salt=0):
        self.lay = layout(cfg, name)
        self.n = len(self.lay)
        self.pos0 = np.array([p for p, _ in self.lay], np.int32)
        self.rows = np.array([r for _, r in self.lay], np.int32)
        self.row0 = np.concatenate([[0], np.cumsum(self.rows)[:-1]]).astype(int)
        self.R = int(self.rows.sum())
        assert self.R == int(name.rstrip("ab")) and self.pos0.max() + 1 <= cfg.seq_len
        rng = np.random.default_rng([7, self.R, salt])
        self.tokens = [rng.integers(2, cfg.vocab_size, r).astype(np.int32) for r in self.rows]
        for t, p in zip(self.tokens, self.pos0):
            if p == 0:
                t[0] = 1
        self.temp = np.array([SETTINGS[j % 7][0] for j in range(self.n)], np.float32)
        self.topp = np.array([SETTINGS[j % 7][1] for j in range(self.n)], np.float32)
        self.coins = []
        for j, r in enumerate(self.rows):
            c = rng.random(int(r), np.float32)
            if SETTINGS[j % 7][2] is not None:
                c[:] = SETTINGS[j % 7][2]
            self.coins.append(c)

    def sampled(self):
        return dict(temperature=self.temp, top_p=self.topp, coin_lists=self.coins)


def snap(states, cfg):
    """(logits, key cache, value cache) of every runstate, as bits"""
    return [(bits(s.logits()),) + tuple(bits(x) for x in caches(s, cfg)) for s in states]


def assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        for name, p, q in zip(("logits", "key cache", "value cache"), x, y):
            assert np.array_equal(p, q), (what, "sequence", i, name)


def close(*groups):
    for g in groups:
        for s in g:
            s.close()


def matrix(s0, R):
    """the call's logits matrix through the hook, as bits"""
    return np.stack([bits(s0.verify_logits(r)) for r in range(R)])


def own_rows(s, cfg, pos0, rows):
    return [bits(x[:, pos0:pos0 + rows]) for x in caches(s, cfg)]


# ---- 1. one-row identity ----
ONE_ROW = [("small", 17), ("small", 33), ("small", 128), ("hs64", 33), ("streams-2048", 33)]


@pytest.mark.parametrize("shape,n", ONE_ROW, ids=[f"{s}-{n}" for s, n in ONE_ROW])
def test_one_row_per_sequence_is_the_wide_step_bit_for_bit(gpu, ck, worlds, shape, n):
    wd = worlds(shape)
    cfg = wd.cfg
    L = cfg.seq_len
    rng = np.random.default_rng([3, n])
    pos = np.array(([L - 1, 0, 63, 64, 65, 127, 128] + rng.integers(0, L, n).tolist())[:n], np.int32)
    tok = rng.integers(2, cfg.vocab_size, n).astype(np.int32)
    tok[pos == 0] = 1
    a, b = wd.fork(pos), wd.fork(pos)
    nxts, acc = gpu.verify_wide(a, [[t] for t in tok], pos, wd.w)
    ref = gpu.transformer_wide(b, tok, pos, wd.w)
    assert np.array_equal(np.concatenate(nxts), ref), (shape, n)
    assert acc.shape == (n,) and not acc.any()
    assert_same(snap(a, cfg), snap(b, cfg), (shape, n))
    close(a, b)


# ---- 2. parity ----
PARITY = [("small", "17"), ("small", "33a"), ("small", "128"), ("hs64", "33b"), ("streams-2048", "33a")]


def oracle_rows(orc, wd, case):
    """the oracle's logits of every row: one pass over the prefix as far as the deepest sequence's first position, then the
    sequences in order of falling first position (a step rewrites row `pos` before it reads rows 0 .. pos, and a sequence
    reads nothing of the prefix at or beyond its own first position)"""
    m = orc.Model(wd.cfg.as_i32(), wd.blob, False)
    for p in range(int(case.pos0.max())):
        m.transformer(int(wd.prefix[p]), p)
    z = [None] * case.R
    for j in sorted(range(case.n), key=lambda j: -int(case.pos0[j])):
        for i, t in enumerate(case.tokens[j]):
            z[case.row0[j] + i] = m.transformer(int(t), int(case.pos0[j]) + i).copy()
    m.close()
    return np.stack(z)


@pytest.mark.parametrize("shape,name", PARITY, ids=[f"{s}-{n}" for s, n in PARITY])
def test_parity_with_l2z_verify_and_the_oracle(gpu, ck, orc, worlds, shape, name):
    wd = worlds(shape)
    cfg, case = wd.cfg, Case(wd.cfg, name)
    states = wd.fork(case.pos0)
    nxts, _ = gpu.verify_wide(states, case.tokens, case.pos0, wd.w)
    z = np.stack([states[0].verify_logits(r) for r in range(case.R)])
    worst = worst_kv = 0.0
    for j in range(case.n):
        p0, rows, r0 = int(case.pos0[j]), int(case.rows[j]), case.row0[j]
        twin = wd.fork([p0])[0]
        ref_next, _ = twin.verify(case.tokens[j], p0, wd.w)
        for i in range(rows):
            ref = twin.verify_logits(i)
            err, bar = float(np.abs(z[r0 + i] - ref).max()), bar_of(ref)
            worst = max(worst, err / bar)
            assert err <= 2 * bar, (shape, name, j, i, err, bar)
            assert int(nxts[j][i]) == int(np.argmax(z[r0 + i])), (shape, name, j, i)   # l2z_argmax's rule on its own logits
        for got, want in zip(caches(states[j], cfg), caches(twin, cfg)):
            d = float(np.abs(got[:, p0:p0 + rows] - want[:, p0:p0 + rows]).max())
            worst_kv = max(worst_kv, d)
            np.testing.assert_allclose(got[:, p0:p0 + rows], want[:, p0:p0 + rows], rtol=KV_TOL, atol=KV_TOL)
        twin.close()
    print(f"verify_wide {shape} {name}: worst logit error {worst:.3f} of the bar against l2z_verify, worst KV difference {worst_kv:.2e}")
    if (shape, name) == ("small", "33a"):
        zo = oracle_rows(orc, wd, case)
        worst_o = 0.0
        for r in range(case.R):
            err, bar = float(np.abs(z[r] - zo[r]).max()), bar_of(zo[r])
            worst_o = max(worst_o, err / bar)
            assert err <= bar, (shape, name, "oracle", r, err, bar)
        print(f"verify_wide {shape} {name}: worst logit error {worst_o:.3f} of the bar against the oracle")
    close(states)


# ---- 3. the verdict, 4. the draw ----
def settle(gpu, wd, states, case, kw):
    """guesses built from the call's own out_next, one more right row per call: afterwards every guess of every sequence is
    the token the row before it draws, so every sequence accepts all its rows"""
    toks = [t.copy() for t in case.tokens]
    for k in range(1, int(case.rows.max())):
        nxts, _ = gpu.verify_wide(states, toks, case.pos0, wd.w, **kw)
        for t, nx in zip(toks, nxts):
            if k < t.size:
                t[k] = nx[k - 1]
    return toks


def host_accept(tokens, nxt):
    a = 0
    while a + 1 < len(tokens) and tokens[a + 1] == nxt[a]:
        a += 1
    return a


@pytest.mark.parametrize("shape,name", [("small", "33a"), ("small", "128"), ("hs64", "33b")])
def test_verdict_and_draw(gpu, ck, worlds, shape, name):
    wd = worlds(shape)
    cfg, case = wd.cfg, Case(wd.cfg, name, salt=1)
    kw = case.sampled()
    states = wd.fork(case.pos0)
    toks = settle(gpu, wd, states, case, kw)
    # sequences with more than one row: every third keeps all its guesses, the next breaks a guess half way (a sequence of
    # two rows has only the first to break), the third its first guess
    want, k = [], 0
    for j in range(case.n):
        rows = int(case.rows[j])
        if rows == 1:
            want.append(0)
            continue
        cut = (None, max(1, rows // 2), 1)[k % 3]
        k += 1
        if cut is not None:
            toks[j][cut] = (toks[j][cut] + 1 - 2) % (cfg.vocab_size - 2) + 2   # another id, not BOS
        want.append(rows - 1 if cut is None else cut - 1)
    nxts, acc = gpu.verify_wide(states, toks, case.pos0, wd.w, **kw)
    kinds = set()
    z = matrix(states[0], case.R)
    with pytest.raises(gpu.L2ZError) as e:
        states[1].verify_logits(0)
    assert e.value.code == gpu.ERR_STATE
    with pytest.raises(gpu.L2ZError):
        states[0].verify_logits(case.R)
    for j in range(case.n):
        rows, r0 = int(case.rows[j]), case.row0[j]
        a = host_accept(toks[j], nxts[j])
        assert int(acc[j]) == a == want[j], (shape, name, j, int(acc[j]), a, want[j])
        kinds.add("none" if a == 0 and rows > 1 else "all" if a == rows - 1 and rows > 1 else "some" if rows > 1 else "one")
        assert np.array_equal(bits(states[j].logits()), z[r0 + a]), (shape, name, j, "the runstate's logits are row row0 + a")
        if case.temp[j] == 0.0:
            assert states[j].argmax() == int(nxts[j][a]), (shape, name, j)
    assert {"none", "some", "all"} <= kinds, kinds
    # the draw: every sampled row's id is l2z_sample_batch's from the same logits, temperature, top_p and coin
    spare = [gpu.RunState(cfg) for _ in range(16)]
    rows_s = [(j, i) for j in range(case.n) if case.temp[j] > 0 for i in range(int(case.rows[j]))]
    assert len(rows_s) >= case.R // 2
    for g in range(0, len(rows_s), 16):
        grp = rows_s[g:g + 16]
        for s, (j, i) in zip(spare, grp):
            s.write_logits(z[case.row0[j] + i].view(np.float32))
        ids = gpu.sample_batch(spare[:len(grp)], [case.temp[j] for j, _ in grp], [case.topp[j] for j, _ in grp],
                               [case.coins[j][i] for j, i in grp])
        for (j, i), t in zip(grp, ids):
            assert int(t) == int(nxts[j][i]), (shape, name, "draw", j, i)
    # the runstates go on: a wide step at the next position, and l2z_verify at an earlier one
    nxt_tok = np.array([nxts[j][acc[j]] for j in range(case.n)], np.int32)
    then = case.pos0 + acc + 1
    room = then < cfg.seq_len
    idx = np.flatnonzero(room)
    gpu.transformer_wide([states[j] for j in idx], nxt_tok[idx], then[idx], wd.w)
    states[1].verify(toks[1][:2], int(case.pos0[1]), wd.w)
    states[1].verify_logits(1)   # ... and the hook is that call's again
    close(states, spare)


# ---- 5. neighbour invariance ----
@pytest.mark.parametrize("name", ["33a", "128"])
def test_neighbour_invariance_and_run_to_run(gpu, ck, worlds, name):
    wd = worlds("small")
    cfg, case = wd.cfg, Case(wd.cfg, name, salt=2)
    kw = case.sampled()
    rng = np.random.default_rng([SEED["small"], 22])

    def result(states, nxts, acc):
        out = []
        for j, s in enumerate(states):
            out.append((nxts[j].copy(), np.array([acc[j]]), bits(s.logits())) + tuple(bits(x) for x in caches(s, cfg)))
        return out

    first_states = wd.fork(case.pos0)
    first = result(first_states, *gpu.verify_wide(first_states, case.tokens, case.pos0, wd.w, **kw))
    rows_first = matrix(first_states[0], case.R)
    again = wd.fork(case.pos0)
    second = result(again, *gpu.verify_wide(again, case.tokens, case.pos0, wd.w, **kw))
    for j in range(case.n):
        for x, y in zip(first[j], second[j]):
            assert np.array_equal(x, y), (name, "run to run", j)
    assert np.array_equal(rows_first, matrix(again[0], case.R))
    other_base = gpu.RunState(cfg)
    other_base.prefill(np.array([1] + rng.integers(2, cfg.vocab_size, cfg.seq_len - 2).tolist(), np.int32), 0, wd.w)
    for part in (0, 1):   # the sequences watched in this run: every second one; the others change tokens, coins and caches
        kept = np.arange(case.n) % 2 == part
        toks = [t if kept[j] else rng.integers(2, cfg.vocab_size, t.size).astype(np.int32) for j, t in enumerate(case.tokens)]
        coins = [c if kept[j] else rng.random(c.size, np.float32) for j, c in enumerate(case.coins)]
        states = [forked(gpu, wd.base if kept[j] else other_base, int(case.pos0[j]), wd.garbage) for j in range(case.n)]
        got = result(states, *gpu.verify_wide(states, toks, case.pos0, wd.w, temperature=case.temp, top_p=case.topp,
                                              coin_lists=coins))
        rows_got = matrix(states[0], case.R)
        for j in np.flatnonzero(kept):
            for what, x, y in zip(("next", "accepted", "logits", "key cache", "value cache"), first[j], got[j]):
                assert np.array_equal(x, y), (name, "neighbours", part, int(j), what)
            r0, rows = case.row0[j], int(case.rows[j])
            assert np.array_equal(rows_first[r0:r0 + rows], rows_got[r0:r0 + rows]), (name, "neighbours", part, int(j), "rows")
        close(states)
    close(first_states, again, [other_base])


# ---- 6. causality ----
def test_guesses_behind_a_row_do_not_reach_it(gpu, ck, worlds):
    wd = worlds("small")
    cfg, case = wd.cfg, Case(wd.cfg, "128", salt=3)
    a, b = wd.fork(case.pos0), wd.fork(case.pos0)
    gpu.verify_wide(a, case.tokens, case.pos0, wd.w)
    za = matrix(a[0], case.R)
    toks, cut = [t.copy() for t in case.tokens], {}
    for j in range(case.n):   # every second sequence of several rows: the guesses behind row i change
        rows = int(case.rows[j])
        if rows > 1 and j % 2 == 1:
            i = cut[j] = (rows - 1) // 2
            toks[j][i + 1:] = (toks[j][i + 1:] - 2 + 5) % (cfg.vocab_size - 2) + 2
    assert len(cut) >= 4 and any(i > 0 for i in cut.values())
    gpu.verify_wide(b, toks, case.pos0, wd.w)
    zb = matrix(b[0], case.R)
    for j in range(case.n):
        rows, r0, p0 = int(case.rows[j]), case.row0[j], int(case.pos0[j])
        same = cut.get(j, rows - 1) + 1   # rows 0 .. same - 1 must not move
        assert np.array_equal(za[r0:r0 + same], zb[r0:r0 + same]), (j, "logits rows up to the changed guess")
        for x, y in zip(own_rows(a[j], cfg, p0, same), own_rows(b[j], cfg, p0, same)):
            assert np.array_equal(x, y), (j, "KV rows up to the changed guess")
        if j in cut:   # ... and the test looks: the rows behind do move
            assert not np.array_equal(za[r0 + same:r0 + rows], zb[r0 + same:r0 + rows]), j
            for x, y in zip(own_rows(a[j], cfg, p0 + same, rows - same), own_rows(b[j], cfg, p0 + same, rows - same)):
                assert not np.array_equal(x, y), j
    close(a, b)


# ---- 7. footprint ----
def test_footprint_only_the_calls_rows_of_the_calls_runstates(gpu, ck, worlds):
    wd = worlds("small")
    cfg, case = wd.cfg, Case(wd.cfg, "33a", salt=4)
    states = wd.fork(case.pos0)
    absent = wd.fork([0, 61, cfg.seq_len - 4])
    before, before_absent = snap(states, cfg), snap(absent, cfg)
    gpu.verify_wide(states, case.tokens, case.pos0, wd.w, **case.sampled())
    after = snap(states, cfg)
    for j in range(case.n):
        keep = np.ones(cfg.seq_len, bool)
        keep[case.pos0[j]:case.pos0[j] + case.rows[j]] = False
        for what, was, got in zip(("key", "value"), before[j][1:], after[j][1:]):
            assert np.array_equal(got[:, keep], was[:, keep]), (j, what, "a row outside the sequence's own changed")
            assert not np.array_equal(got[:, ~keep], was[:, ~keep]), (j, what, "the sequence's rows were not written")
    assert_same(snap(absent, cfg), before_absent, "runstates absent from the call")
    close(states, absent)


# ---- 8. refusals ----
def test_contract_refusals_change_nothing(gpu, ck):
    c = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    c2 = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=48)
    odd = ck.Config(dim=64, hidden_dim=174, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)   # l2z_prefill refuses
    w, w2, w_odd = gpu.Weights(c, None, False, seed=4), gpu.Weights(c2, None, False, seed=4), gpu.Weights(odd, None, False, seed=4)
    ss = [gpu.RunState(c) for _ in range(gpu.WIDE_MAX + 1)]
    foreign, odd_ss = gpu.RunState(c2), [gpu.RunState(odd) for _ in range(2)]
    comm = gpu.Comm(0, 2, None, 0, emulated=True)
    shard = gpu.RunState(c, comm)   # one rank of two, on this device
    for i, s in enumerate(ss[:3]):
        s.prefill(np.array([3 + i, 4, 5], np.int32), 0, w)

    assert gpu.verify_wide(ss[:3], [[6, 7], [8], [9, 10, 11]], 3, w)[1].shape == (3,)   # the scratch and a hook matrix exist

    def snap3():
        return [(np.concatenate([bits(x).ravel() for x in caches(s, c)]), bits(s.logits())) for s in ss[:3]] + \
               [(bits(ss[0].verify_logits(r)).copy(), np.zeros(0)) for r in range(6)]
    before = snap3()
    L = gpu.lib()
    i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    nan, inf = float("nan"), float("inf")

    def call(states, lists, pos0, temp=None, topp=None, coins=None, n=None, null=(), weights=None, cfg=None):
        n = len(states) if n is None else n
        arr = (C.c_void_p * max(len(states), 1))(*[s.h for s in states])
        nt = np.array([len(t) for t in lists] + [0], np.int32)
        t = np.array([x for t in lists for x in t] + [0], np.int32)
        p = np.array(list(pos0) + [0], np.int32)
        fl = [None if v is None else np.ascontiguousarray(v, np.float32) for v in (temp, topp, coins)]
        nxt, acc = np.zeros(t.size + 1, np.int32), np.zeros(len(states) + 1, np.int32)
        args = [n, t.ctypes.data_as(i32), nt.ctypes.data_as(i32), p.ctypes.data_as(i32)] + \
               [None if v is None else v.ctypes.data_as(f32) for v in fl] + \
               [C.byref(cfg or ss[0].cfg), arr, (weights or w).h, nxt.ctypes.data_as(i32), acc.ctypes.data_as(i32)]
        for k in null:
            args[k] = C.cast(None, i32) if k in (1, 2, 3, 10, 11) else None
        return L.l2z_verify_wide(*args)

    a, b = ss[0], ss[1]
    two = ([a, b], [[1, 7], [1, 8, 9]], [3, 3])
    ok = dict(temp=[1.0, 0.0], topp=[0.9, 0.9], coins=[0.5, 0.25, 0.5, 0.5, 0.5])
    INV, ST = gpu.ERR_INVALID, gpu.ERR_STATE
    assert call([a], [[1]], [3], n=0) == INV
    assert call(ss, [[1]] * len(ss), [3] * len(ss)) == INV                           # n = 129
    assert call(ss[:9], [[1] * 15] * 8 + [[1] * 9], [3] * 9) == INV                  # R = 129
    assert call([a, b], [[1] * 17, [1]], [3, 3]) == INV                              # n_tokens[0] = 17
    assert call([a, b], [[1], []], [3, 3]) == INV                                    # n_tokens[1] = 0
    assert call([a, b, a], [[1], [1], [1]], [3, 3, 3]) == INV                        # the same runstate twice
    assert call([a, foreign], [[1], [1]], [3, 3]) == INV                             # a runstate of another config
    assert call(*two, weights=w2) == INV                                             # weights of another config
    assert call([a, shard], [[1, 7], [1, 8, 9]], [3, 3]) == INV                      # a shard as states[1]
    assert call([shard, a], [[1, 7], [1, 8, 9]], [3, 3]) == INV                      # a shard as states[0]
    assert call(odd_ss, [[1, 7], [1, 8, 9]], [3, 3], cfg=odd_ss[0].cfg, weights=w_odd) == INV   # dims l2z_prefill refuses
    for k in (1, 2, 3, 7, 8, 9, 10, 11):                                             # tokens, n_tokens, pos0, config, states, w, outs
        assert call(*two, null=(k,), **ok) == INV, k
    # the sampler's rules
    for bad in (nan, inf, -1.0):
        assert call(*two, **dict(ok, temp=[1.0, bad])) == INV, bad
    for bad in (-0.1, 1.5, nan):
        assert call(*two, **dict(ok, topp=[0.9, bad])) == INV, bad
    assert call(*two, **dict(ok, topp=None)) == INV                                  # top_p NULL beside temperature
    assert call(*two, **dict(ok, coins=None)) == INV
    for bad in (1.0, -0.1, nan):
        assert call(*two, **dict(ok, coins=[0.5, bad, 0.5, 0.5, 0.5])) == INV, bad    # the sampled sequence's LAST coin
    # positions and tokens
    assert call([a, b], [[1, 7], [1, 8, 9]], [-1, 3], **ok) == ST
    assert call([a, b], [[1, 7], [1, 8, 9]], [3, c.seq_len - 2], **ok) == ST          # 30 + 3 rows > seq_len
    assert call([a, b], [[1, 7], [1, 8, 9]], [c.seq_len, 3], **ok) == ST
    assert call([a, b], [[1, 7], [1, 8, c.vocab_size]], [3, 3], **ok) == ST
    assert call([a, b], [[1, -1], [1, 8, 9]], [3, 3]) == ST
    for (k0, l0), (k1, l1) in zip(before, snap3()):
        assert np.array_equal(k0, k1) and np.array_equal(l0, l1)
    # the bookkeeping is as before: a wide step at the old position still succeeds ...
    gpu.transformer_wide([a, b], [1, 1], [3, 3], w)
    # ... and the same arguments are accepted once they are right: a greedy sequence's coins are not read, the last position
    # is reachable, all greedy needs no sampler argument, 128 rows of 128 sequences and of 8
    assert call([a, b], [[1, 7], [1, 8, 9]], [3, c.seq_len - 3], **dict(ok, coins=[0.5, 0.25, nan, 7.0, -1.0])) == gpu.OK
    assert not np.array_equal(bits(a.logits()), before[0][1])
    assert call(*two) == gpu.OK
    assert call(*two, temp=[0.0, 0.0], topp=[1.0, 1.0]) == gpu.OK                    # (no coins: no sequence draws)
    assert call(ss[:gpu.WIDE_MAX], [[1]] * gpu.WIDE_MAX, [0] * gpu.WIDE_MAX, temp=[0.5] * gpu.WIDE_MAX,
                topp=[0.9] * gpu.WIDE_MAX, coins=[0.5] * gpu.WIDE_MAX) == gpu.OK
    assert call(ss[:8], [[1] * 16] * 8, [0] * 8) == gpu.OK
    for s in ss + [foreign, shard] + odd_ss:
        s.close()
    comm.close()
    for x in (w, w2, w_odd):
        x.close()


# ---- 9. speculate_wide ----
SPEC_SEED, SPEC_N, SPEC_STEPS, SPEC_PROMPT = 23, 40, 16, 3


def spec_prompts(cfg):
    rng = np.random.default_rng([SPEC_SEED, 31])
    return [rng.integers(2, cfg.vocab_size, SPEC_PROMPT).tolist() for _ in range(SPEC_N)]


def test_speculate_wide_greedy(gpu, ck, worlds):
    """`small` (seed 23), 40 sequences of 3 prompt tokens run to 16 tokens.  k = 0: generate_wide's ids bit for bit (test 1's
    identity, step after step).  k = 3 with a drafter that replays the reference run: 40 x 4 rows are asked for, so the
    guesses are trimmed to 128 rows a call; every sequence's ids equal the reference run's up to the first position whose
    top-two margin in the reference run is under twice the bar -- beyond it the forms may part.  Checked with the CPU
    oracle alone before any GPU run: at this shape, weights seed 23, prompt seed (23, 31) and length, 37 of the 40
    sequences keep every margin of their run above twice the bar and so are compared over their whole length (the smallest
    margin of all is 0.30 of the bar, the median sequence's smallest 42 bars); the test asks for three quarters."""
    wd = worlds("small")
    cfg, w, n, steps, P = wd.cfg, wd.w, SPEC_N, SPEC_STEPS, SPEC_PROMPT
    prompts = spec_prompts(cfg)

    def fresh():
        return [gpu.RunState(cfg) for _ in range(n)]
    # the reference run, from entry points that stood before: the prompts as speculate_wide feeds them, then wide steps
    ref_states = fresh()
    for g in range(0, n, 16):
        gpu.prefill_batch(ref_states[g:g + 16], [np.array([1] + p, np.int32) for p in prompts[g:g + 16]], 0, w)
    first = np.concatenate([gpu.argmax_batch(ref_states[g:g + 16]) for g in range(0, n, 16)]).astype(np.int32)
    assert not (first == 1).any()

    def margins(states):
        out = []
        for s in states:
            z = s.logits()
            two = np.partition(z.astype(np.float64), -2)[-2:]
            out.append((two[1] - two[0]) / bar_of(z))
        return np.array(out)
    marg = [margins(ref_states)]
    ids, tok = [first], first
    for k in range(steps - P - 1):
        tok = gpu.transformer_wide(ref_states, tok, np.full(n, P + 1 + k, np.int32), w)
        ids.append(tok)
        marg.append(margins(ref_states))
    ref = np.stack(ids).T            # [n, steps - P]: sequence j's generated ids
    marg = np.stack(marg).T
    assert not (ref == 1).any(), "a sequence drew BOS: the live set would shrink"
    twin = fresh()
    for g in range(0, n, 16):
        gpu.prefill_batch(twin[g:g + 16], [np.array([1] + p, np.int32) for p in prompts[g:g + 16]], 0, w)
    assert np.array_equal(gpu.generate_wide(twin, first, P + 1, w, steps - P - 1).T, ref[:, 1:])
    # k = 0
    a = fresh()
    out, stats = gpu.speculate_wide(a, w, prompts, steps, 0)
    for j in range(n):
        assert np.array_equal(out[j], np.array(prompts[j] + ref[j].tolist(), np.int32)), j
    assert stats["calls"] == steps - P - 1 and set(stats["rows_per_call"]) == {n}
    assert_same(snap(a, cfg), snap(ref_states, cfg), "k = 0")
    # k = 3, the reference run replayed
    full = {tuple(prompts[j]): prompts[j] + ref[j].tolist() for j in range(n)}

    def replay(hist, kk):
        seq = full[tuple(int(t) for t in hist[1:P + 1])]
        return np.array(seq[len(hist) - 1:len(hist) - 1 + kk], np.int32)
    b = fresh()
    out, stats = gpu.speculate_wide(b, w, prompts, steps, 3, replay)
    assert max(stats["rows_per_call"]) <= gpu.WIDE_MAX and stats["rows_per_call"][0] == gpu.WIDE_MAX
    assert stats["calls"] < steps - P - 1 and stats["accepted"] > 0
    whole = 0
    for j in range(n):
        under = np.flatnonzero(marg[j] < 2.0)
        upto = P + (int(under[0]) if under.size else ref.shape[1])
        whole += not under.size
        assert np.array_equal(out[j][:upto], np.array(full[tuple(prompts[j])][:upto], np.int32)), (j, upto)
    print(f"speculate_wide k=3: {whole} of {n} sequences compared over their whole length; {stats['calls']} calls, "
          f"rows per call {stats['rows_per_call']}")
    assert whole >= 0.75 * n, "vacuous: too few sequences compared over their whole length"
    close(ref_states, twin, a, b)


def test_speculate_wide_sampled_emits_each_calls_accepted_rows(gpu, ck, worlds, monkeypatch):
    """coin_stream coins, position-indexed: every call's rows of a sequence take the coins of the generated tokens they
    stand for, the ids a call emits are its out_next[row0 .. row0 + a], and the positions advance by a + 1"""
    wd = worlds("small")
    cfg, w, n, steps, P = wd.cfg, wd.w, 20, SPEC_STEPS, SPEC_PROMPT
    prompts = spec_prompts(cfg)[:n]
    coins = [gpu.coin_stream(100 + j, steps) for j in range(n)]
    temp = np.array([SETTINGS[j % 7][0] for j in range(n)], np.float32)
    topp = np.array([SETTINGS[j % 7][1] for j in range(n)], np.float32)
    calls, real = [], gpu.verify_wide

    def recorder(states, lists, pos0s, w_, temperature=None, top_p=None, coin_lists=None):
        nxts, accs = real(states, lists, pos0s, w_, temperature, top_p, coin_lists)
        calls.append(([id(s) for s in states], [list(t) for t in lists], list(pos0s), [np.array(c) for c in coin_lists],
                      [x.copy() for x in nxts], accs.copy()))
        return nxts, accs
    monkeypatch.setattr(gpu, "verify_wide", recorder)
    states = [gpu.RunState(cfg) for _ in range(n)]
    out, stats = gpu.speculate_wide(states, w, prompts, steps, 3, temperature=temp, top_p=topp, coins=coins)
    monkeypatch.undo()
    assert calls and stats["calls"] == len(calls)
    where = {id(s): j for j, s in enumerate(states)}
    emitted = {j: list(out[j][:P + 1]) for j in range(n)}   # the prompt and the first draw (l2z_sample_batch after the prefill)
    at = {j: P + 1 for j in range(n)}
    for handles, lists, pos0s, clists, nxts, accs in calls:
        assert sum(len(t) for t in lists) <= gpu.WIDE_MAX and max(len(t) for t in lists) <= 4
        for h, t, p, c, nx, a in zip(handles, lists, pos0s, clists, nxts, accs):
            j = where[h]
            assert p == at[j] and t[0] == emitted[j][-1], (j, "a call goes on where the last one stopped")
            assert np.array_equal(c[:len(t)], coins[j][p - P:p - P + len(t)]), (j, "the rows' coins are their positions'")
            assert int(a) == host_accept(t, nx)
            take = [int(x) for x in nx[:int(a) + 1]][:steps - at[j]]
            if 1 in take:
                take = take[:take.index(1) + 1]
            emitted[j] += take
            at[j] += len(take)
    for j in range(n):
        assert np.array_equal(out[j], np.array(emitted[j], np.int32)), j
        assert len(out[j]) == steps or out[j][-1] == 1
    close(states)
