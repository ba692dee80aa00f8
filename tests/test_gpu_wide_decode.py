"""l2z_transformer_wide on the GPU: one decode step for up to 128 sequences, one runstate each, as one chunk of the ragged
prompt pass with the position-split decode attention (wide_decode.hip).

For every row the call must leave what l2z_transformer(tokens[i], pos[i]) on states[i] leaves.  Checked against the CPU
oracle's stepped pass at THE BAR of tests/test_gpu_parity.py (LOGIT_ATOL + LOGIT_RTOL * max |z|); token ids where the
oracle's margin exceeds the bar; three consecutive steps against oracle models of their own (they read the scattered KV
rows) and, secondarily, against l2z_transformer_batch in groups of 16 on forked copies.  Neighbour invariance, the cache
footprint and the contract are checked bit for bit.

The oracle is kept cheap: every sequence of a shape continues ONE common prefix at its own depth.  The GPU prefills the
prefix once and forks it to each runstate; the oracle steps the prefix once and then visits the sequences in order of
FALLING position -- its step rewrites row `pos` before it reads rows 0 .. pos, so a shallower sequence still sees the
prefix intact below its own position.  One such pass per shape serves every n: a batch of n is the first n sequences.
The widest shape's pass is a recorded one (GOLDEN below).
"""
import ctypes as C
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_parity import LOGIT_ATOL, LOGIT_RTOL
from test_gpu_prefill_batch import SHAPES as PROMPT_SHAPES, bits, caches

pytestmark = pytest.mark.gpu

KV_TOL = 2e-5   # a KV row against l2z_transformer_batch's
WIDE = 128
# The partial parts of the wide attention, which no prompt-pass shape reaches: a block serves up to 4 query heads of one kv
# head.  `small`'s widths (every GEMM form takes them) with 6 heads on 2 kv heads -- kv_mul 3: one part of 3 heads in a
# block made for 4 -- and on 1 kv head -- kv_mul 6: two parts, 4 + 2.
PARTS = dict(dim=288, hidden_dim=768, n_layers=2, n_heads=6, vocab_size=1024, seq_len=160)
SHAPES = dict(PROMPT_SHAPES, **{"kvmul3": dict(PARTS, n_kv_heads=2), "kvmul6": dict(PARTS, n_kv_heads=1)})
# seeds picked on the CPU with the oracle alone: at most 5 % of a case's rows have a top-2 margin under the bar
SEED = {"small": 23, "gqa": 23, "hs64": 23, "mqa-256": 23, "streams-2048": 23, "kvmul3": 23, "kvmul6": 23}

# (shape, n, L2Z_PF_X3): both sides of every GEMM-form switch-over on `small`, 33 and 128 on every other shape
PARITY = ([("small", n, 1) for n in (1, 16, 17, 32, 33, 64, 65, 128)] +
          [(s, n, 1) for s in ("gqa", "hs64", "mqa-256", "kvmul3", "kvmul6") for n in (33, 128)] +
          [("streams-2048", n, x3) for x3 in (1, 2) for n in (33, 128)])


def bar_of(z):
    return LOGIT_ATOL + LOGIT_RTOL * float(np.abs(z).max())


def plan(ck, shape):
    """the shape's config, weights blob, common prefix (seq_len - 1 tokens), and WIDE (position, token) rows: the edges of
    the attention's segments and of the context first, so that every batch of 7 or more rows holds them"""
    cfg = ck.Config(**SHAPES[shape])
    rng = np.random.default_rng([SEED[shape], 1])
    L = cfg.seq_len
    prefix = np.array([1] + rng.integers(2, cfg.vocab_size, L - 2).tolist(), np.int32)
    edges = [p for p in (L - 1, 0, 63, 64, 65, 127, 128) if p < L]
    pos = np.array(edges + rng.integers(0, L, WIDE - len(edges)).tolist(), np.int32)
    tok = rng.integers(2, cfg.vocab_size, WIDE).astype(np.int32)
    tok[pos == 0] = 1
    return cfg, prefix, pos, tok


def oracle_rows(ck, orc, shape, rows):
    """the oracle's logits of the given rows of plan(shape): one pass over the prefix as far as the deepest of them, then
    the rows in order of falling position"""
    cfg, prefix, pos, tok = plan(ck, shape)
    blob = ck.synth_blob(cfg, False, seed=SEED[shape])
    m = orc.Model(cfg.as_i32(), blob, False)
    for p in range(max(int(pos[i]) for i in rows)):
        m.transformer(int(prefix[p]), p)
    z = {}
    for i in sorted(rows, key=lambda i: -int(pos[i])):
        z[i] = m.transformer(int(tok[i]), int(pos[i]))
    m.close()
    return np.stack([z[i] for i in rows])


# streams-2048: 559 prefix positions of a model 2048 wide take the oracle close to a minute, so its pass is RECORDED
# (scripts/wide_golden.py writes the file; tests/test_wide_golden.py re-derives its shallow rows without a GPU)
GOLDEN = {"streams-2048": os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_ref_streams_2048.npz")}


@functools.lru_cache(maxsize=None)
def reference(ck, orc, shape):
    """the oracle's logits, argmax and top-2 margin of every row of plan(shape)"""
    if shape in GOLDEN:
        _, prefix, pos, tok = plan(ck, shape)
        g = np.load(GOLDEN[shape])
        assert np.array_equal(g["prefix"], prefix) and np.array_equal(g["pos"], pos) and np.array_equal(g["tok"], tok) and \
            int(g["seed"]) == SEED[shape], "the recorded pass is another plan's: run scripts/wide_golden.py"
        z = g["z"]
    else:
        z = oracle_rows(ck, orc, shape, list(range(WIDE)))
    two = np.partition(z.astype(np.float64), -2, axis=1)[:, -2:]
    return z, np.argmax(z, axis=1), two[:, 1] - two[:, 0]


class World:
    """a shape on the GPU: its weights, the prefix in a base runstate, and WIDE runstates forked at the rows' depths"""

    def __init__(self, gpu, ck, shape):
        self.cfg, self.prefix, self.pos, self.tok = plan(ck, shape)
        self.w = gpu.Weights(self.cfg, ck.synth_blob(self.cfg, False, seed=SEED[shape]), False)
        self.base = gpu.RunState(self.cfg)
        self.base.prefill(self.prefix, 0, self.w)
        self.states = [forked(gpu, self.base, int(p)) for p in self.pos]

    def close(self):
        for s in self.states + [self.base]:
            s.close()
        self.w.close()


def forked(gpu, base, depth, garbage=None):
    """a runstate holding base's rows 0 .. depth - 1; garbage: another runstate's whole cache underneath (stale rows)"""
    s = gpu.RunState(base.cfg)
    if garbage is not None:
        gpu.runstate_fork(s, garbage, base.cfg.seq_len)
    gpu.runstate_fork(s, base, depth)
    s.synchronize()
    return s


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


@pytest.mark.parametrize("shape,n,x3", PARITY, ids=[f"{s}-{n}-x3_{x}" for s, n, x in PARITY])
def test_one_step_against_the_oracle(gpu, ck, orc, options, worlds, shape, n, x3):
    """rows 0 .. n - 1 of the shape's plan in one call (a step rewrites row pos[i] before anything reads it, so the
    runstates serve every n)"""
    options(L2Z_PF_X3=x3)
    z, top, margin = reference(ck, orc, shape)
    wd = worlds(shape)
    if n >= 7:
        assert {p for p in (wd.cfg.seq_len - 1, 0, 63, 64, 65, 127, 128) if p < wd.cfg.seq_len} <= set(wd.pos[:n].tolist())
    nxt = gpu.transformer_wide(wd.states[:n], wd.tok[:n], wd.pos[:n], wd.w)
    worst, under = 0.0, 0
    for i in range(n):
        lg = wd.states[i].logits()
        bar = bar_of(z[i])
        err = float(np.abs(lg - z[i]).max())
        worst = max(worst, err / bar)
        assert err <= bar, (shape, n, i, int(wd.pos[i]), err, bar)
        assert int(nxt[i]) == int(np.argmax(lg)), (shape, n, i)   # the device's argmax is l2z_argmax's of these logits
        if margin[i] > bar:
            assert int(nxt[i]) == int(top[i]), (shape, n, i)
        else:
            under += 1
    print(f"wide {shape} n={n} x3={x3}: worst error {worst:.3f} of its bar; {under} of {n} rows under the margin rule")
    assert under <= 0.05 * n, "vacuous: too many rows left out of the token comparison"


def test_without_out_next_the_call_leaves_the_same_logits(gpu, ck, worlds):
    wd = worlds("small")
    n = 33
    gpu.transformer_wide(wd.states[:n], wd.tok[:n], wd.pos[:n], wd.w)
    with_next = [bits(s.logits()) for s in wd.states[:n]]
    assert gpu.transformer_wide(wd.states[:n], wd.tok[:n], wd.pos[:n], wd.w, want_next=False) is None
    for i, s in enumerate(wd.states[:n]):
        assert np.array_equal(bits(s.logits()), with_next[i]), i


@pytest.mark.parametrize("shape", ["small", "hs64"])
def test_three_steps_against_oracles_of_their_own_and_the_batched_step(gpu, ck, orc, worlds, shape):
    """33 sequences, three consecutive wide steps on fixed tokens: steps two and three read the KV rows the steps before
    scattered.  The first, the last, the deepest and the shallowest sequence against an oracle model each; the whole batch
    against l2z_transformer_batch in groups of 16 on forked copies; every other cache row bit-unchanged."""
    wd = worlds(shape)
    cfg, n, steps = wd.cfg, 33, 3
    rng = np.random.default_rng([SEED[shape], 2])
    pos0 = rng.integers(1, 130, n).astype(np.int32)
    pos0[5], pos0[20] = 0, 130                      # the shallowest; the deepest crosses into a third segment
    toks = rng.integers(2, cfg.vocab_size, (steps, n)).astype(np.int32)
    toks[0, pos0 == 0] = 1
    chosen = sorted({0, n - 1, 20, 5})
    blob = ck.synth_blob(cfg, False, seed=SEED[shape])

    def oracle(i):
        m = orc.Model(cfg.as_i32(), blob, False)
        for p in range(int(pos0[i])):
            m.transformer(int(wd.prefix[p]), p)
        out = [m.transformer(int(toks[k, i]), int(pos0[i]) + k) for k in range(steps)]
        m.close()
        return out
    with ThreadPoolExecutor(4) as ex:   # the oracle's calls release the GIL
        ref = dict(zip(chosen, ex.map(oracle, chosen)))
    wide = [forked(gpu, wd.base, int(p)) for p in pos0]
    copies = [forked(gpu, wd.base, int(p)) for p in pos0]
    before = [caches(s, cfg) for s in wide]
    worst = 0.0
    for k in range(steps):
        gpu.transformer_wide(wide, toks[k], pos0 + k, wd.w)
        for g in range(0, n, 16):
            gpu.transformer_batch(copies[g:g + 16], toks[k, g:g + 16], pos0[g:g + 16] + k, wd.w)
        for i in range(n):
            lg = wide[i].logits()
            if i in ref:
                bar = bar_of(ref[i][k])
                err = float(np.abs(lg - ref[i][k]).max())
                worst = max(worst, err / bar)
                assert err <= bar, (shape, "oracle", i, k, err, bar)
            other = copies[i].logits()
            d = float(np.abs(lg - other).max())
            assert d <= 2 * bar_of(other), (shape, "batched step", i, k, d)
    print(f"wide {shape} three steps: worst error {worst:.3f} of its bar")
    for i in range(n):
        keep = np.ones(cfg.seq_len, bool)
        keep[pos0[i]:pos0[i] + steps] = False
        for got, was, cp in zip(caches(wide[i], cfg), before[i], caches(copies[i], cfg)):
            assert np.array_equal(bits(got[:, keep]), bits(was[:, keep])), (shape, i, "a row outside the steps' changed")
            np.testing.assert_allclose(got[:, ~keep], cp[:, ~keep], rtol=KV_TOL, atol=KV_TOL)
    # the runstates go on: the batched step, l2z_argmax
    gpu.transformer_batch(wide[:16], toks[0, :16], pos0[:16] + steps, wd.w)
    gpu.transformer_batch(copies[:16], toks[0, :16], pos0[:16] + steps, wd.w)
    for a, b in zip(wide[:16], copies[:16]):
        assert float(np.abs(a.logits() - b.logits()).max()) <= 2 * bar_of(b.logits())
        assert a.argmax() == int(np.argmax(a.logits()))
    for s in wide + copies:
        s.close()


@pytest.mark.parametrize("shape,n", [("small", 33), ("small", 128), ("hs64", 33), ("kvmul3", 33), ("kvmul6", 33)])
def test_neighbour_invariance_and_run_to_run(gpu, ck, worlds, shape, n):
    """a fixed n and a fixed place: row i's logits and KV row are the same bits whatever tokens, depths and prefixes the
    other rows hold, whatever stale rows its own cache holds beyond pos[i] -- and from run to run"""
    wd = worlds(shape)
    cfg, w = wd.cfg, wd.w
    rng = np.random.default_rng([SEED[shape], 3, n])
    L = cfg.seq_len
    pos, tok = wd.pos[:n].copy(), wd.tok[:n].copy()

    def result(states, p):
        out = []
        for s, q in zip(states, p):
            k, v = caches(s, cfg)
            out.append((bits(s.logits()), bits(k[:, q]), bits(v[:, q])))
        return out

    gpu.transformer_wide(wd.states[:n], tok, pos, w)
    first = result(wd.states[:n], pos)
    gpu.transformer_wide(wd.states[:n], tok, pos, w)
    for i, (a, b) in enumerate(zip(first, result(wd.states[:n], pos))):
        for x, y in zip(a, b):
            assert np.array_equal(x, y), (shape, n, "run to run", i)
    # another prefix for the neighbours, and garbage for the stale rows: every row of a cache holds other contents
    other_base, garbage = gpu.RunState(cfg), gpu.RunState(cfg)
    other_base.prefill(np.array([1] + rng.integers(2, cfg.vocab_size, L - 2).tolist(), np.int32), 0, w)
    garbage.prefill(rng.integers(2, cfg.vocab_size, L).astype(np.int32), 0, w)
    for part in (0, 1):   # the rows kept in this run: every second one; the others change token, depth and prefix
        kept = np.arange(n) % 2 == part
        p2 = np.where(kept, pos, (pos + rng.integers(1, L, n)) % L).astype(np.int32)
        if part == 0:
            p2[1] = L - 1   # a neighbour deeper than every kept row: the grid's segment extent grows
        t2 = np.where(kept, tok, rng.integers(2, cfg.vocab_size, n)).astype(np.int32)
        states = [forked(gpu, wd.base if kept[i] else other_base, int(p2[i]), garbage) for i in range(n)]
        gpu.transformer_wide(states, t2, p2, w)
        got = result(states, p2)
        for i in np.flatnonzero(kept):
            for x, y in zip(first[i], got[i]):
                assert np.array_equal(x, y), (shape, n, "neighbours", int(i))
        for s in states:
            s.close()
    other_base.close()
    garbage.close()


def test_generate_wide_equals_the_step_by_step_loop(gpu, ck, worlds):
    wd = worlds("small")
    n, steps = 20, 8
    pos0 = np.minimum(wd.pos[:n], wd.cfg.seq_len - steps).astype(np.int32)
    a = [forked(gpu, wd.base, int(p)) for p in pos0]
    b = [forked(gpu, wd.base, int(p)) for p in pos0]
    ids = gpu.generate_wide(a, wd.tok[:n], pos0, wd.w, steps)
    assert ids.shape == (steps, n)
    tok = wd.tok[:n].copy()
    for k in range(steps):
        gpu.transformer_wide(b, tok, pos0 + k, wd.w, want_next=False)
        tok = np.array([s.argmax() for s in b], np.int32)   # l2z_argmax on the host's side of the loop
        assert np.array_equal(ids[k], tok), k
    for s in a + b:
        s.close()


def test_contract_refusals_change_nothing(gpu, ck):
    c = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    w = gpu.Weights(c, None, False, seed=4)
    ss = [gpu.RunState(c) for _ in range(WIDE + 1)]
    for i, s in enumerate(ss[:3]):
        s.prefill(np.array([3 + i, 4, 5], np.int32), 0, w)

    def snap():
        return [(np.concatenate([bits(x).ravel() for x in caches(s, c)]), bits(s.logits())) for s in ss[:3]]
    before = snap()
    L = gpu.lib()
    i32 = C.POINTER(C.c_int32)

    def call(states, toks, pos, n=None, out=True, null=None):
        n = len(states) if n is None else n
        arr = (C.c_void_p * max(len(states), 1))(*[s.h for s in states])
        t, p = np.array(toks, np.int32), np.array(pos, np.int32)
        nxt = np.zeros(max(len(states), 1), np.int32)
        args = [n, t.ctypes.data_as(i32), p.ctypes.data_as(i32), C.byref(ss[0].cfg), arr, w.h,
                nxt.ctypes.data_as(i32) if out else None]
        if null is not None:
            args[null] = C.cast(None, i32) if null in (1, 2) else None
        return L.l2z_transformer_wide(*args)

    a, b = ss[0], ss[1]
    assert call([a], [1], [3], n=0) == gpu.ERR_INVALID
    assert call(ss, [1] * (WIDE + 1), [3] * (WIDE + 1)) == gpu.ERR_INVALID          # n = 129
    assert call([a, b, a], [1, 1, 1], [3, 3, 3]) == gpu.ERR_INVALID                 # the same runstate twice
    assert call([a, b], [1, 1], [3, c.seq_len]) == gpu.ERR_STATE
    assert call([a, b], [1, 1], [-1, 3]) == gpu.ERR_STATE
    assert call([a, b], [1, c.vocab_size], [3, 3]) == gpu.ERR_STATE
    assert call([a, b], [-1, 1], [3, 3], out=False) == gpu.ERR_STATE
    for k in (1, 2, 3, 4, 5):
        assert call([a, b], [1, 1], [3, 3], null=k) == gpu.ERR_INVALID, k
    for (k0, l0), (k1, l1) in zip(before, snap()):
        assert np.array_equal(k0, k1) and np.array_equal(l0, l1)
    # ... and the same arguments are accepted once they are right, 128 runstates too
    assert call([a, b], [1, 1], [3, 3]) == gpu.OK
    assert not np.array_equal(bits(a.logits()), before[0][1])
    assert call(ss[:WIDE], [1] * WIDE, [0] * WIDE) == gpu.OK
    for s in ss:
        s.close()
    w.close()
