"""l2z_step_mixed on the GPU: prompt chunks and decode rows as ONE chunk of the ragged prompt pass, the multi-row sequences
through the prompt attention, the one-row sequences through the position-split decode attention, the classifier on the last
rows only (mixed_step.hip, wide_host.cpp), and binding.serve, the continuous-batching loop on top.

What the header promises is checked as it is stated: ALL-ONE-ROW IDENTITY with l2z_transformer_wide, PROMPTS-ONLY IDENTITY of
the KV rows with l2z_prefill_batch, NEIGHBOUR INVARIANCE, THE DRAW, PAGED == contiguous and the footprint bit for bit
(np.array_equal); PARITY of the last rows' logits against the CPU oracle on `small` at THE BAR of tests/test_gpu_parity.py
(LOGIT_ATOL + LOGIT_RTOL * max |z|), against the two-call path (l2z_prefill_batch for the multi-row sequences, then
l2z_transformer_wide for the rest, on forked twins) within twice that, KV rows within 2e-5 -- the margins the wide family's
tests use between two GPU forms.

Every runstate starts as a fork of ONE prefilled prefix at its own depth over a cache full of another sequence's rows
(World.fork of tests/test_gpu_verify_wide.py).

The layouts.  The elements the mixed layouts are to hold -- one-row sequences at positions 0, 63, 64 and seq_len - 1, a
2-row prompt, a 64-row and a 65-row prompt from position 0, a slice of 70 rows or more from position 60 (it crosses 64 and
128), a slice ending on seq_len - 1 -- add up to 205 rows and more, so the layouts of 17, 33 and 129 rows cannot hold them
all.  As in tests/test_gpu_verify_wide.py the large layouts (257: just past the split-K forms' last chunk length, and 512)
hold every one, and the small ones hold what fits: ALL of them the four one-row sequences, the 2-row prompt and a slice from
position 60 that crosses 64 (17: 11 rows; 33: 20 rows, and 7 rows ending on seq_len - 1; 129: the whole 70-row slice from 60,
which crosses 128 too, beside a 53-row prompt from position 0).  The sequences stand in a shuffled order, so a decode row's
ordinal, its row and its sequence slot all differ.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_parity import LOGIT_ATOL, LOGIT_RTOL
from test_gpu_prefill_batch import bits, caches
from test_gpu_verify_wide import KV_TOL, World, assert_same, bar_of, close, snap
from test_gpu_wide_decode import SEED, SHAPES, forked
from test_gpu_wide_run import SETTINGS

pytestmark = pytest.mark.gpu

PAGE = 64


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


def layout(cfg, R):
    """[(pos0, rows)] of the mixed layout of R rows, shuffled"""
    L = cfg.seq_len
    lay = [(0, 1), (63, 1), (64, 1), (L - 1, 1), (5, 2)]
    lay += {17: [(60, 11)],
            33: [(60, 20), (L - 7, 7)],
            129: [(0, 53), (60, 70)],
            257: [(0, 64), (0, 65), (60, 70), (L - 52, 52)],
            512: [(0, 64), (0, 65), (60, 75), (L - 40, 40), (0, 100), (30, 100)] +
                 [(int(p), 1) for p in np.random.default_rng(11).integers(0, L, 62)]}[R]
    assert sum(r for _, r in lay) == R
    order = np.random.default_rng([R, 3]).permutation(len(lay))
    return [lay[i] for i in order]


class Case:
    """a layout on a shape: positions, row counts, tokens, and every sequence's draw (SETTINGS[j % 7], ONE coin each)"""

    def __init__(self, cfg, lay, salt=0):
        self.lay = lay
        self.n = len(lay)
        self.pos0 = np.array([p for p, _ in lay], np.int32)
        self.rows = np.array([r for _, r in lay], np.int32)
        self.R = int(self.rows.sum())
        rng = np.random.default_rng([9, self.R, salt])
        self.tokens = [rng.integers(2, cfg.vocab_size, r).astype(np.int32) for r in self.rows]
        for t, p in zip(self.tokens, self.pos0):
            if p == 0:
                t[0] = 1
        self.temp = np.array([SETTINGS[j % 7][0] for j in range(self.n)], np.float32)
        self.topp = np.array([SETTINGS[j % 7][1] for j in range(self.n)], np.float32)
        self.coins = rng.random(self.n, np.float32)
        for j in range(self.n):
            if SETTINGS[j % 7][2] is not None:
                self.coins[j] = SETTINGS[j % 7][2]
        self.multi = [j for j in range(self.n) if self.rows[j] > 1]
        self.single = [j for j in range(self.n) if self.rows[j] == 1]

    def sampled(self):
        return dict(temperature=self.temp, top_p=self.topp, coins=self.coins)


def sample_16s(gpu, states, temp, topp, coins):
    """l2z_sample_batch over the runstates' logits, in groups of 16"""
    out = []
    for g in range(0, len(states), 16):
        out.append(gpu.sample_batch(states[g:g + 16], temp[g:g + 16], topp[g:g + 16], coins[g:g + 16]))
    return np.concatenate(out)


def own_rows(s, cfg, pos0, rows):
    return [bits(x[:, pos0:pos0 + rows]) for x in caches(s, cfg)]


def code_of(gpu, fn):
    with pytest.raises(gpu.L2ZError) as e:
        fn()
    return e.value.code


# ---- 1. all-one-row identity ----
ONE_ROW = [("small", 1, 1), ("small", 17, 1), ("small", 33, 1), ("small", 128, 1), ("hs64", 33, 1), ("kvmul6", 33, 1),
           ("streams-2048", 33, 1), ("streams-2048", 128, 2)]


@pytest.mark.parametrize("shape,n,x3", ONE_ROW, ids=[f"{s}-{n}-x3_{x}" for s, n, x in ONE_ROW])
def test_all_one_row_is_the_wide_step_bit_for_bit(gpu, worlds, options, shape, n, x3):
    options(L2Z_PF_X3=x3)
    wd = worlds(shape)
    cfg = wd.cfg
    L = cfg.seq_len
    rng = np.random.default_rng([4, n])
    pos = np.array(([63] if n == 1 else [L - 1, 0, 63, 64, 65, 127, 128] + rng.integers(0, L, n).tolist())[:n], np.int32)
    tok = rng.integers(2, cfg.vocab_size, n).astype(np.int32)
    tok[pos == 0] = 1
    temp = np.array([SETTINGS[j % 7][0] for j in range(n)], np.float32)
    topp = np.array([SETTINGS[j % 7][1] for j in range(n)], np.float32)
    coins = rng.random(n, np.float32)
    a, b, c = wd.fork(pos), wd.fork(pos), wd.fork(pos)
    got = gpu.step_mixed(a, [[t] for t in tok], pos, wd.w)                                         # greedy
    got_s = gpu.step_mixed(c, [[t] for t in tok], pos, wd.w, temperature=temp, top_p=topp, coins=coins)
    ref = gpu.transformer_wide(b, tok, pos, wd.w)
    assert np.array_equal(got, ref), (shape, n)
    assert_same(snap(a, cfg), snap(b, cfg), (shape, n, "greedy"))
    assert_same(snap(c, cfg), snap(b, cfg), (shape, n, "sampled"))
    assert np.array_equal(got_s, sample_16s(gpu, b, temp, topp, coins)), (shape, n, "the draw")
    close(a, b, c)


# ---- 2. prompts-only identity ----
PROMPTS = [("small", 1), ("hs64", 1), ("streams-2048", 1), ("streams-2048", 2), ("kvmul6", 1)]


@pytest.mark.parametrize("shape,x3", PROMPTS, ids=[f"{s}-x3_{x}" for s, x in PROMPTS])
def test_prompts_only_writes_the_kv_rows_of_prefill_batch_bit_for_bit(gpu, worlds, options, shape, x3):
    options(L2Z_PF_X3=x3)
    wd = worlds(shape)
    cfg = wd.cfg
    L = cfg.seq_len
    lay = [(0, 2), (0, 64), (0, 65), (60, 70), (L - 9, 9), (10, 33)]
    case = Case(cfg, lay)
    # the identity holds while l2z_prefill_batch runs the rows as ONE chunk, as this call always does
    assert gpu.prefill_plan(case.R, cfg) == [case.R], gpu.prefill_plan(case.R, cfg)
    a, b = wd.fork(case.pos0), wd.fork(case.pos0)
    gpu.step_mixed(a, case.tokens, case.pos0, wd.w)
    gpu.prefill_batch(b, case.tokens, case.pos0, wd.w)
    for j in range(case.n):
        for name, x, y in zip(("key cache", "value cache"), caches(a[j], cfg), caches(b[j], cfg)):
            assert np.array_equal(bits(x), bits(y)), (shape, j, name)
        za, zb = a[j].logits(), b[j].logits()
        assert float(np.abs(za - zb).max()) <= bar_of(zb), (shape, j)   # the parity bar itself
    close(a, b)


# ---- 3. parity ----
PARITY = ([("small", R, 1) for R in (17, 33, 129, 257, 512)] + [("hs64", 33, 1), ("hs64", 512, 1), ("kvmul6", 33, 1),
          ("kvmul6", 512, 1), ("streams-2048", 129, 1), ("streams-2048", 33, 2), ("streams-2048", 512, 2)])


def oracle_last_rows(orc, wd, case):
    """the oracle's logits of every sequence's LAST row: one pass over the prefix as far as the deepest first position, then
    the sequences in order of falling first position (oracle_rows of tests/test_gpu_verify_wide.py)"""
    m = orc.Model(wd.cfg.as_i32(), wd.blob, False)
    for p in range(int(case.pos0.max())):
        m.transformer(int(wd.prefix[p]), p)
    z = [None] * case.n
    for j in sorted(range(case.n), key=lambda j: -int(case.pos0[j])):
        for i, t in enumerate(case.tokens[j]):
            z[j] = m.transformer(int(t), int(case.pos0[j]) + i)
        z[j] = z[j].copy()
    m.close()
    return z


@pytest.mark.parametrize("shape,R,x3", PARITY, ids=[f"{s}-{r}-x3_{x}" for s, r, x in PARITY])
def test_parity_with_the_two_call_path_and_the_oracle(gpu, orc, worlds, options, shape, R, x3):
    options(L2Z_PF_X3=x3)
    wd = worlds(shape)
    cfg, case = wd.cfg, Case(wd.cfg, layout(wd.cfg, R))
    assert {0, 63, 64, cfg.seq_len - 1} <= {int(case.pos0[j]) for j in case.single}
    assert any(p == 60 and p + r > 64 for p, r in case.lay) and (5, 2) in case.lay
    if R >= 257:
        assert {(0, 64), (0, 65)} <= set(case.lay) and any(p == 60 and r >= 70 for p, r in case.lay)
        assert any(r > 1 and p + r == cfg.seq_len for p, r in case.lay)
    states, twins = wd.fork(case.pos0), wd.fork(case.pos0)
    nxt = gpu.step_mixed(states, case.tokens, case.pos0, wd.w)
    gpu.prefill_batch([twins[j] for j in case.multi], [case.tokens[j] for j in case.multi], case.pos0[case.multi], wd.w)
    gpu.transformer_wide([twins[j] for j in case.single], [int(case.tokens[j][0]) for j in case.single],
                         case.pos0[case.single], wd.w)
    worst = worst_kv = 0.0
    for j in range(case.n):
        p0, rows = int(case.pos0[j]), int(case.rows[j])
        z, ref = states[j].logits(), twins[j].logits()
        err, bar = float(np.abs(z - ref).max()), bar_of(ref)
        worst = max(worst, err / bar)
        print(f"step_mixed {shape} R={R} sequence {j} (pos0 {p0}, {rows} rows): logit error {err:.3e}, bar {bar:.3e}")
        assert err <= 2 * bar, (shape, R, j, err, bar)
        assert int(nxt[j]) == int(np.argmax(z)), (shape, R, j)   # l2z_argmax's rule on its own logits
        for got, want in zip(caches(states[j], cfg), caches(twins[j], cfg)):
            worst_kv = max(worst_kv, float(np.abs(got[:, p0:p0 + rows] - want[:, p0:p0 + rows]).max()))
            np.testing.assert_allclose(got[:, p0:p0 + rows], want[:, p0:p0 + rows], rtol=KV_TOL, atol=KV_TOL)
    print(f"step_mixed {shape} R={R}: worst logit error {worst:.3f} of the bar against the two-call path, worst KV difference {worst_kv:.2e}")
    if shape == "small":
        zo = oracle_last_rows(orc, wd, case)
        worst_o = 0.0
        for j in range(case.n):
            err, bar = float(np.abs(states[j].logits() - zo[j]).max()), bar_of(zo[j])
            worst_o = max(worst_o, err / bar)
            assert err <= bar, (shape, R, "oracle", j, err, bar)
        print(f"step_mixed {shape} R={R}: worst logit error {worst_o:.3f} of the bar against the oracle")
    close(states, twins)


# ---- 4. neighbour invariance and run to run, 5. the draw ----
@pytest.mark.parametrize("shape", ["small", "hs64", "kvmul6"])
def test_neighbour_invariance_run_to_run_and_the_draw(gpu, worlds, shape):
    wd = worlds(shape)
    cfg = wd.cfg
    case, other = Case(cfg, layout(cfg, 33)), Case(cfg, layout(cfg, 33), salt=1)
    kept = list(range(0, case.n, 2))   # these sequences keep their tokens; the others change tokens AND caches

    def run(tokens, states):
        ids = gpu.step_mixed(states, tokens, case.pos0, wd.w, **case.sampled())
        got = [(int(ids[j]), bits(states[j].logits())) + tuple(own_rows(states[j], cfg, 0, int(case.pos0[j] + case.rows[j])))
               for j in range(case.n)]
        return ids, got

    a, a2 = wd.fork(case.pos0), wd.fork(case.pos0)
    ids, ra = run(case.tokens, a)
    _, ra2 = run(case.tokens, a2)
    for j in range(case.n):   # run to run
        assert ra[j][0] == ra2[j][0] and all(np.array_equal(x, y) for x, y in zip(ra[j][1:], ra2[j][1:])), (shape, "rerun", j)
    # THE DRAW: the ids are l2z_sample_batch's from the logits as read back
    assert np.array_equal(ids, sample_16s(gpu, a, case.temp, case.topp, case.coins)), shape
    assert {float(c) for c in case.coins} >= {0.0, float(SETTINGS[5][2])} or case.n < 7
    # the neighbours: other tokens, the OTHER prefix in their caches (garbage's rows below, base's as the stale rows);
    # the kept sequences: nothing stale beyond their own rows (a fresh cache's zeros instead of garbage's rows)
    b = [forked(gpu, wd.base, int(case.pos0[j])) if j in kept else forked(gpu, wd.garbage, int(case.pos0[j]), wd.base)
         for j in range(case.n)]
    mixed_tokens = [case.tokens[j] if j in kept else other.tokens[j] for j in range(case.n)]
    _, rb = run(mixed_tokens, b)
    for j in kept:
        assert ra[j][0] == rb[j][0] and all(np.array_equal(x, y) for x, y in zip(ra[j][1:], rb[j][1:])), (shape, "neighbours", j)
    assert any(ra[j][0] != rb[j][0] or not np.array_equal(ra[j][1], rb[j][1]) for j in range(case.n) if j not in kept)
    close(a, a2, b)


# ---- 6. paged ----
def attached(s):
    p = s.pages()
    return p[p >= 0]


# every mixed layout on `small`; 512 rows are 73 paged sequences in one table; streams-2048 is the shape on which the paged flash
# form and the decode combine both write the bf16 planes (L2Z_PF_X3 1 and 2)
PAGED = ([("small", R, 1) for R in (17, 33, 129, 257, 512)] + [("hs64", 257, 1), ("kvmul6", 33, 1), ("streams-2048", 129, 1),
         ("streams-2048", 33, 2), ("streams-2048", 512, 2)])


@pytest.mark.parametrize("shape,R,x3", PAGED, ids=[f"{s}-{r}-x3_{x}" for s, r, x in PAGED])
def test_paged_runstates_equal_contiguous_ones_bit_for_bit(gpu, worlds, options, shape, R, x3):
    options(L2Z_PF_X3=x3)
    wd = worlds(shape)
    cfg, case = wd.cfg, Case(wd.cfg, layout(wd.cfg, R))
    need = sum((int(p + r) + PAGE - 1) // PAGE for p, r in case.lay)
    pool = gpu.KvPool(cfg, need + 12)
    # recycled pages in an order that is neither ascending nor adjacent: six dummies of two pages each, written by mixed
    # calls of their own (so the pages hold stale rows), given back out of order
    dummies = [gpu.RunState(cfg, pool=pool) for _ in range(6)]
    gpu.step_mixed(dummies, [np.r_[1, np.arange(2, PAGE + 2)].astype(np.int32)] * 6, 0, wd.w)
    for i in (0, 3, 1, 4, 2, 5):
        dummies[i].close()
    ref = wd.fork(case.pos0)
    got = [gpu.RunState(cfg, pool=pool) for _ in range(case.n)]
    for s, p in zip(got, case.pos0):
        gpu.runstate_fork(s, wd.base, int(p))
    ids_ref = gpu.step_mixed(ref, case.tokens, case.pos0, wd.w, **case.sampled())
    ids_got = gpu.step_mixed(got, case.tokens, case.pos0, wd.w, **case.sampled())
    lists = [attached(s) for s in got]
    assert any(len(a) >= 2 and np.any(np.diff(a) < 0) for a in lists), lists
    assert any(len(a) >= 2 and np.any(np.abs(np.diff(a)) > 1) for a in lists), lists
    assert [len(a) for a in lists] == [(int(p + r) + PAGE - 1) // PAGE for p, r in case.lay]
    assert np.array_equal(ids_ref, ids_got)
    for j in range(case.n):
        end = int(case.pos0[j] + case.rows[j])
        assert np.array_equal(bits(ref[j].logits()), bits(got[j].logits())), (shape, R, j)
        for x, y in zip(own_rows(ref[j], cfg, 0, end), own_rows(got[j], cfg, 0, end)):
            assert np.array_equal(x, y), (shape, R, j)
    close(ref, got)
    assert pool.info()["n_free"] == need + 12
    pool.close()


def test_a_call_short_of_pages_is_refused_with_nothing_attached(gpu, worlds):
    wd = worlds("small")
    cfg = wd.cfg
    pool = gpu.KvPool(cfg, 4)
    got = [gpu.RunState(cfg, pool=pool) for _ in range(3)]
    rng = np.random.default_rng(6)
    first = [np.r_[1, rng.integers(2, cfg.vocab_size, 59)].astype(np.int32) for _ in range(3)]
    gpu.step_mixed(got, first, 0, wd.w)   # positions 0 .. 59: a page each, one is left

    def state():
        return pool.info()["n_free"], [s.pages().tolist() for s in got], [bits(s.logits()) for s in got]
    before = state()
    assert before[0] == 1
    # sequence 0 decodes inside its page, sequence 1 crosses into a second page, sequence 2's slice into a second too: two
    # pages missing, one free
    lists = [[5], rng.integers(2, cfg.vocab_size, 5).astype(np.int32), rng.integers(2, cfg.vocab_size, 30).astype(np.int32)]
    assert code_of(gpu, lambda: gpu.step_mixed(got, lists, [60, 60, 60], wd.w)) == gpu.ERR_OOM
    after = state()
    assert after[0] == before[0] and after[1] == before[1]
    assert all(np.array_equal(x, y) for x, y in zip(before[2], after[2]))
    gpu.step_mixed(got[:2], lists[:2], [60, 60], wd.w)   # what the pool does hold is accepted
    assert pool.info()["n_free"] == 0
    close(got)
    pool.close()


# ---- 7. footprint and refusals ----
def test_footprint_and_refusals(gpu, worlds):
    wd = worlds("small")
    cfg = wd.cfg
    L, V = cfg.seq_len, cfg.vocab_size
    case = Case(cfg, layout(cfg, 33))
    states, bystander = wd.fork(case.pos0), wd.fork([100])[0]
    before, by_before = snap(states, cfg), snap([bystander], cfg)
    gpu.step_mixed(states, case.tokens, case.pos0, wd.w, **case.sampled())
    assert_same(snap([bystander], cfg), by_before, "the bystander")
    for j, s in enumerate(states):   # only the call's rows of the call's runstates change
        lo, hi = int(case.pos0[j]), int(case.pos0[j] + case.rows[j])
        keep = np.ones(L, bool)
        keep[lo:hi] = False
        for x, old in zip(caches(s, cfg), before[j][1:]):
            assert np.array_equal(bits(x)[:, keep], old[:, keep]), ("footprint", j)
            assert not np.array_equal(bits(x)[:, lo:hi], old[:, lo:hi]), ("the rows were written", j)
    # refusals: nothing changes, whatever is refused
    states = wd.fork(case.pos0)
    many = wd.fork([3] * 129)
    pool = gpu.KvPool(cfg, 2)
    paged = gpu.RunState(cfg, pool=pool)
    held = snap(states, cfg)
    pages_before = (pool.info()["n_free"], paged.pages().tolist())
    ok = dict(states=states, tokens=case.tokens, pos0=case.pos0, kw=case.sampled())

    def call(**ch):
        a = dict(ok, **ch)
        return code_of(gpu, lambda: gpu.step_mixed(a["states"], a["tokens"], a["pos0"], wd.w, **a["kw"]))

    def with_seq(j, **ch):
        """the valid call with sequence j's tokens / pos0 / control replaced"""
        tokens, pos0, kw = list(case.tokens), case.pos0.copy(), {k: v.copy() for k, v in case.sampled().items()}
        if "tokens" in ch:
            tokens[j] = np.asarray(ch["tokens"], np.int32)
        if "pos0" in ch:
            pos0[j] = ch["pos0"]
        for k in ("temperature", "top_p", "coins"):
            if k in ch:
                kw[k][j] = ch[k]
        return dict(tokens=tokens, pos0=pos0, kw=kw)
    multi, samp = case.multi[0], next(j for j in range(case.n) if case.temp[j] > 0)
    INVALID, STATE = gpu.ERR_INVALID, gpu.ERR_STATE
    assert call(states=[], tokens=[], pos0=[], kw={}) == INVALID                                   # n = 0
    assert call(states=many, tokens=[[2]] * 129, pos0=[3] * 129, kw={}) == INVALID                 # n = 129
    assert call(states=states[:2], tokens=[np.full(300, 2, np.int32), np.full(213, 2, np.int32)], pos0=[0, 0], kw={}) == INVALID   # R = 513
    assert call(**with_seq(multi, tokens=[])) == INVALID                                           # an n_tokens[j] = 0
    assert call(states=states[:-1] + [states[0]]) == INVALID                                       # duplicate runstates
    assert call(states=states[:-1] + [paged]) == INVALID                                           # mixed kinds
    assert call(**with_seq(samp, temperature=-1.0)) == INVALID
    assert call(**with_seq(samp, temperature=np.nan)) == INVALID
    assert call(**with_seq(samp, top_p=1.5)) == INVALID
    assert call(**with_seq(samp, coins=1.0)) == INVALID
    assert call(kw=dict(temperature=case.temp, top_p=case.topp, coins=None)) == INVALID             # no coins beside a temperature > 0
    assert call(**with_seq(multi, pos0=L - int(case.rows[multi]) + 1)) == STATE                    # a position past seq_len
    assert call(**with_seq(multi, pos0=-1)) == STATE
    bad = case.tokens[multi].copy()
    bad[-1] = V
    assert call(**with_seq(multi, tokens=bad)) == STATE                                            # a token outside the vocabulary
    assert_same(snap(states, cfg), held, "after the refusals")
    assert (pool.info()["n_free"], paged.pages().tolist()) == pages_before
    # a later valid call is accepted, and gives what the same call gave before
    twin = wd.fork(case.pos0)
    ids = gpu.step_mixed(states, case.tokens, case.pos0, wd.w, **case.sampled())
    ids2 = gpu.step_mixed(twin, case.tokens, case.pos0, wd.w, **case.sampled())
    assert np.array_equal(ids, ids2)
    assert_same(snap(states, cfg), snap(twin, cfg), "the valid call after the refusals")
    close(states, twin, many, [bystander, paged])
    pool.close()


# ---- 8. the loop ----
# binding.serve on `small`: 8 greedy requests, prompts of 1 .. 90 tokens, max_new 8 .. 16, at most 4 sequences in flight, 48
# rows per step, a pool of 4 pages (the requests need 1, 2, 1, 2, 1, 1, 2, 1).
# The prompts' seeds were picked on the CPU with the oracle alone (one per request: the first seed for which every emitted
# position of that request has a top-2 margin of at least twice the parity bar); the test recomputes the condition.
LOOP_LENS = [1, 90, 17, 64, 33, 5, 70, 48]
LOOP_NEW = [8, 16, 12, 9, 16, 10, 14, 11]
LOOP_SEEDS = [0, 0, 1, 0, 0, 0, 0, 0]
BOS = 1


def loop_prompt(cfg, j):
    rng = np.random.default_rng([LOOP_SEEDS[j], j])
    return np.array([BOS] + rng.integers(2, cfg.vocab_size, LOOP_LENS[j] - 1).tolist(), np.int32)


def oracle_greedy(orc, cfg, blob, prompt, max_new):
    """the oracle's greedy continuation of a prompt as serve cuts it (BOS, max_new, seq_len), and the smallest
    margin / bar over the emitted positions"""
    m = orc.Model(cfg.as_i32(), blob, False)
    for p, t in enumerate(prompt):
        z = m.transformer(int(t), p)
    ids, tightest, pos = [], np.inf, len(prompt)
    while True:
        two = np.partition(z.astype(np.float64), -2)[-2:]
        tightest = min(tightest, float(two[1] - two[0]) / bar_of(z))
        ids.append(int(np.argmax(z)))
        if ids[-1] == BOS or len(ids) >= max_new or pos >= cfg.seq_len:
            break
        z = m.transformer(ids[-1], pos)
        pos += 1
    m.close()
    return np.array(ids, np.int32), tightest


def test_serve_is_the_oracles_greedy_continuation_and_replays(gpu, orc, worlds):
    wd = worlds("small")
    cfg = wd.cfg
    n = len(LOOP_LENS)
    prompts = [loop_prompt(cfg, j) for j in range(n)]
    with ThreadPoolExecutor(8) as ex:   # the oracle's calls release the GIL
        ref = list(ex.map(lambda j: oracle_greedy(orc, cfg, wd.blob, prompts[j], LOOP_NEW[j]), range(n)))
    for j, (_, tightest) in enumerate(ref):
        assert tightest >= 2.0, f"request {j}: an emitted position has a top-2 margin of {tightest:.2f} bars: pick another seed"
    pool = gpu.KvPool(cfg, 4)
    ids, trace = gpu.serve(list(zip(prompts, LOOP_NEW)), wd.w, pool, max_seqs=4, row_budget=48)
    assert pool.info()["n_free"] == 4
    pool.close()
    # what the trace must show
    started, pages = {}, [(LOOP_LENS[j] + LOOP_NEW[j] + PAGE - 1) // PAGE for j in range(n)]
    slices = mixes = waits = 0
    for k, st in enumerate(trace):
        assert len(st["ids"]) <= 4 and sum(st["n_tokens"]) <= 48
        for i in st["ids"]:
            started.setdefault(i, k)
        slices += any(m >= 2 and p > 0 for m, p in zip(st["n_tokens"], st["pos0"]))
        mixes += any(m == 1 for m in st["n_tokens"]) and any(m >= 2 for m in st["n_tokens"])
        # admission waited: a request had not started, a runstate and rows were to be had, and the step ran without it
        waits += len(started) < n and len(st["ids"]) < 4 and sum(st["n_tokens"]) < 48
    last = {i: max(k for k, st in enumerate(trace) if i in st["ids"]) for i in range(n)}
    assert slices >= 1 and mixes >= 1 and waits >= 1, (slices, mixes, waits)
    assert min(last.values()) < len(trace) - 1                              # a retirement while others go on
    assert any(started[i] > min(last.values()) for i in range(n))           # ... and a request that started after it
    # reuse of pages, read from the trace: a page a retired request held is held later by a request that started after it
    held = {i: set() for i in range(n)}
    for st in trace:
        assert len({p for pg in st["pages"] for p in pg}) == sum(len(pg) for pg in st["pages"]) <= 4   # no page held twice at once
        for i, pg in zip(st["ids"], st["pages"]):
            held[i] |= set(pg)
    assert all(len(held[i]) == pages[i] for i in range(n)), (held, pages)
    assert any(held[i] & held[j] for i in range(n) for j in range(n) if started[j] > last[i])
    assert list(started) == sorted(started)                                 # arrival order
    # the replay: the same layouts through step_mixed on fresh runstates give the same ids bit for bit
    fresh = [gpu.RunState(cfg) for _ in range(n)]
    text = [np.concatenate([prompts[j], ids[j]]) for j in range(n)]
    again = [[] for _ in range(n)]
    for st in trace:
        lists = [text[i][p: p + m] for i, m, p in zip(st["ids"], st["n_tokens"], st["pos0"])]
        nxt = gpu.step_mixed([fresh[i] for i in st["ids"]], lists, st["pos0"], wd.w)
        for i, m, p, t in zip(st["ids"], st["n_tokens"], st["pos0"], nxt):
            if p + m >= LOOP_LENS[i]:
                again[i].append(int(t))
    for j in range(n):
        assert np.array_equal(np.array(again[j], np.int32), ids[j]), ("replay", j)
        assert np.array_equal(ids[j], ref[j][0]), ("oracle", j, ids[j], ref[j][0])   # no exceptions
    close(fresh)
