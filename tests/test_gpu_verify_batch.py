"""l2z_verify_batch on the GPU: the verify pass for the rows of SEVERAL sequences in one sweep of the weights, and the batched
speculative loop on top (binding.verify_batch, binding.speculate_batch).

The references: the single-sequence calls themselves on forked twins of the same states (RunState.verify /
RunState.verify_sample; uint32 compares of the next ids, the accepted count, every logits row, the runstate's logits and
BOTH whole caches -- which also shows that no other cache row was touched); the CPU oracle's stepped pass for values
(logits rtol = atol = 5e-5, KV rows 2e-5: the bars of tests/test_gpu_verify.py); speculate_greedy / speculate_sample on
fresh runstates for the loop.

Models: three of tests/test_gpu_verify.py's table with that file's random token stream per model (the same seeds).
toy_gqa_unshared: context 32, GQA; stories15M: head_size 48, so a lane group is not a power-of-two fit; long_gqa:
head_size 128, kv_mul 2, context 2048, so many segments.  The oracle steps the first ORACLE_DEPTH positions of a stream
only: every sequence that needs the oracle (right guesses, parity) sits below that depth; the deep ones (pos 1000, 2047)
are compared with their twins alone.  Positions are written for long_gqa; a shorter context cuts them to fit."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_verify import NAMES as VERIFY_NAMES
from test_gpu_verify import bits, caches, feed_history, model, np_accept, np_argmax

pytestmark = pytest.mark.gpu

LOGIT_RTOL = 5e-5   # tests/test_gpu_verify.py's bars
LOGIT_ATOL = 5e-5
KV_TOL = 2e-5
SEG = 64  # csrc/batch_decode.h kVerifySeg
NAMES = ("toy_gqa_unshared", "stories15M", "long_gqa")
ORACLE_DEPTH = 640   # covers 5 * SEG + 220 + 16


class Stream:
    """a model, test_gpu_verify.py's random stream over its whole context, and the oracle's stepped pass over the first
    `depth` positions of it; chain(): the oracle's own greedy continuation behind a position of the stream"""

    def __init__(self, ck, orc, name):
        self.name = name
        self.cfg, self.shared, self.blob = model(ck, name)
        c = self.cfg
        rng = np.random.default_rng(1000 + VERIFY_NAMES.index(name))
        self.toks = rng.integers(2, c.vocab_size, size=c.seq_len).astype(np.int32)
        self.depth = min(c.seq_len, ORACLE_DEPTH)
        self.m = orc.Model(c.as_i32(), self.blob, self.shared)
        self.logits = np.empty((self.depth, c.vocab_size), np.float32)
        for p in range(self.depth):
            self.logits[p] = self.m.transformer(int(self.toks[p]), p)
        kvd = c.dim // c.n_heads * c.n_kv_heads
        n = c.n_layers * c.seq_len * kvd
        self.k = self.m.state("key_cache", n).reshape(c.n_layers, c.seq_len, kvd).copy()
        self.v = self.m.state("value_cache", n).reshape(c.n_layers, c.seq_len, kvd).copy()

    def chain(self, pos0, m):
        """g[0 .. m): g[0] = the oracle's argmax after stream[: pos0 + 1], g[i] = its argmax after that and g[: i].  The
        oracle's cache rows behind pos0 are put back afterwards by stepping the stream's tokens again."""
        assert pos0 + m <= self.depth
        g = [np_argmax(self.logits[pos0])]
        for i in range(1, m):
            g.append(np_argmax(self.m.transformer(g[-1], pos0 + i)))
        for p in range(pos0 + 1, pos0 + m):
            self.m.transformer(int(self.toks[p]), p)
        return g


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


# ---- layouts: (pos0, rows, right) per sequence; right = how many leading guesses are the oracle's own continuation --------

def depths_16(seq_len):
    want = [0, SEG - 1, SEG, seq_len - 1, 1, 17, SEG - 2, SEG + 1, 2 * SEG - 1, 2 * SEG, 300, 5 * SEG + 220, 1000, 1023, 1024,
            seq_len - 2]
    out = []
    for p in want + list(range(seq_len)):
        if 0 <= p < seq_len and p not in out:
            out.append(p)
        if len(out) == 16:
            break
    return out


def layouts(seq_len):
    deep = 5 * SEG + 220   # 540: segment 8, rows 540 .. 543
    ragged = [(100, 1, 0), (SEG - 4, 7, 4), (deep, 3, 0), (0, 5, 2)]   # (1, 7, 3, 5) rows; the second straddles position 64
    out = {
        "a_1x16": [(SEG - 8, 16, 5)],
        "b_16x1": [(p, 1, 0) for p in depths_16(seq_len)],
        "c_4x4": [(0, 4, 3), (SEG - 2, 4, 0), (SEG, 4, 1), (deep, 4, 2)],
        "d_ragged": ragged,
        "e_ragged_permuted": [ragged[i] for i in (2, 0, 3, 1)],
    }
    return {k: [(min(p, seq_len - t), t, r) for p, t, r in v] for k, v in out.items()}   # a shorter context cuts them


def sequence_tokens(st, rng, pos0, T, right):
    """(tokens, the accepted count the oracle expects or None): the stream's token at pos0, `right` right guesses, then a
    wrong one and random ones.  right = 0: the stream's own next tokens (random, so wrong almost surely)."""
    c = st.cfg
    if right == 0:
        toks = st.toks[pos0:pos0 + T].copy()
        if pos0 + T > st.depth:
            return toks, None
        return toks, np_accept(toks, [np_argmax(st.logits[pos0 + i]) for i in range(T)])
    right = min(right, T - 1)
    g = st.chain(pos0, right + 1)
    toks = np.empty(T, np.int32)
    toks[0] = st.toks[pos0]
    toks[1:right + 1] = g[:right]
    if right + 1 < T:
        toks[right + 1] = (g[right] - 2 + 1) % (c.vocab_size - 2) + 2   # not the oracle's pick
        toks[right + 2:] = rng.integers(2, c.vocab_size, size=T - right - 2)
    return toks, right


def build(gpu, st, w, layout, by_verify, rng):
    """the layout's runstates with their histories fed, a forked twin of each, the token lists and the expected accepts"""
    c = st.cfg
    states, twins, lists, expect = [], [], [], []
    for pos0, T, right in layout:
        s = gpu.RunState(c)
        feed_history(s, w, st.toks, pos0, by_verify)
        t = gpu.RunState(c)
        gpu.runstate_fork(t, s, pos0)
        toks, a = sequence_tokens(st, rng, pos0, T, right)
        states.append(s); twins.append(t); lists.append(toks); expect.append(a)
    return states, twins, lists, expect


def close_all(*groups):
    for g in groups:
        for s in g:
            s.close()


def same_as_twins(gpu, c, states, twins, lists, nxts, accs, twin_results, what):
    """sequence j of the batched call against the single-sequence call on its twin, bit for bit"""
    r = 0
    for j, (s, t) in enumerate(zip(states, twins)):
        tn, ta = twin_results[j]
        assert nxts[j].tolist() == tn.tolist(), (what, j, "next")
        assert int(accs[j]) == ta, (what, j, "accepted")
        for i in range(len(lists[j])):
            assert np.array_equal(bits(states[0].verify_logits(r + i)), bits(t.verify_logits(i))), (what, j, "logits row", i)
        r += len(lists[j])
        assert np.array_equal(bits(s.logits()), bits(t.logits())), (what, j, "runstate logits")
        for mine, theirs, which in zip(caches(s, c), caches(t, c), ("key", "value")):
            assert np.array_equal(bits(mine), bits(theirs)), (what, j, which + " cache")


# ---- 1. bit-identity with the single-sequence call --------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_verify_batch_is_bitwise_the_single_sequence_call(gpu, streams, weights, name):
    st, w = streams[name], weights[name]
    c = st.cfg
    rng = np.random.default_rng(5)
    expected_seen, got_seen = set(), set()
    for case, (what, layout) in enumerate(layouts(c.seq_len).items()):
        states, twins, lists, expect = build(gpu, st, w, layout, by_verify=(case % 2 == 1), rng=rng)
        nxts, accs = gpu.verify_batch(states, lists, [p for p, _, _ in layout], w)
        twin_results = [t.verify(lists[j], layout[j][0], w) for j, t in enumerate(twins)]
        same_as_twins(gpu, c, states, twins, lists, nxts, accs, twin_results, (name, what))
        for j in range(1, len(states)):   # the matrix is states[0]'s: the others must not serve rows of an older call
            with pytest.raises(gpu.L2ZError) as e:
                states[j].verify_logits(0)
            assert e.value.code == gpu.ERR_STATE
        with pytest.raises(gpu.L2ZError):
            states[0].verify_logits(sum(len(t) for t in lists))
        expected_seen |= {a for a in expect if a is not None}
        got_seen |= {int(a) for a in accs}
        print(f"{name} {what}: expected accepts {expect}, got {accs.tolist()}")
        close_all(states, twins)
    # a condition on the INPUTS, by the oracle's logits: the sequences of a call do not all stop at the same place
    assert len(expected_seen) >= 2, expected_seen
    # ... and the verdict kernel did return different accept lengths (within single calls too: layouts c to e)
    assert len(got_seen) >= 2, got_seen


# ---- 2. sampled mode ---------------------------------------------------------------------------------------------------------

DRAWS = ((0.0, 0.5), (1.0, 0.9), (0.7, 1.0), (1.0, 0.0))   # (temperature, top_p) per sequence; top_p is unused at temperature 0


@pytest.mark.parametrize("name", NAMES)
def test_verify_batch_sampled_is_bitwise_verify_sample(gpu, streams, weights, name):
    st, w = streams[name], weights[name]
    c = st.cfg
    layout = layouts(c.seq_len)["c_4x4"]
    pos0s = [p for p, _, _ in layout]
    states, twins, lists, _ = build(gpu, st, w, layout, by_verify=False, rng=np.random.default_rng(6))
    coins = [gpu.coin_stream(40 + j, len(lists[j])) for j in range(4)]
    temps, tops = [d[0] for d in DRAWS], [d[1] for d in DRAWS]
    nxts, accs = gpu.verify_batch(states, lists, pos0s, w, temps, tops, [None] + coins[1:])   # no coins at temperature 0
    twin_results = [t.verify_sample(lists[j], pos0s[j], w, temps[j], tops[j], coins[j]) for j, t in enumerate(twins)]
    same_as_twins(gpu, c, states, twins, lists, nxts, accs, twin_results, (name, "sampled"))
    close_all(states, twins)


def test_temperature_none_is_the_all_zero_temperature_call(gpu, streams, weights):
    st, w = streams["long_gqa"], weights["long_gqa"]
    c = st.cfg
    layout = layouts(c.seq_len)["d_ragged"]
    pos0s = [p for p, _, _ in layout]
    a, b, lists, _ = build(gpu, st, w, layout, by_verify=False, rng=np.random.default_rng(7))
    n0, a0 = gpu.verify_batch(a, lists, pos0s, w)
    n1, a1 = gpu.verify_batch(b, lists, pos0s, w, 0.0, 0.3, None)
    assert a0.tolist() == a1.tolist() and [x.tolist() for x in n0] == [x.tolist() for x in n1]
    for r in range(sum(len(t) for t in lists)):
        assert np.array_equal(bits(a[0].verify_logits(r)), bits(b[0].verify_logits(r)))
    for s, t in zip(a, b):
        assert np.array_equal(bits(s.logits()), bits(t.logits()))
        for x, y in zip(caches(s, c), caches(t, c)):
            assert np.array_equal(bits(x), bits(y))
    close_all(a, b)


# ---- 3. parity with the oracle's stepped pass ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_verify_batch_meets_the_oracle(gpu, streams, weights, name):
    st, w = streams[name], weights[name]
    c = st.cfg
    layout = [(p, t, 0) for p, t, _ in layouts(c.seq_len)["c_4x4"]]   # every row follows the stream
    states, twins, lists, _ = build(gpu, st, w, layout, by_verify=False, rng=np.random.default_rng(8))
    nxts, accs = gpu.verify_batch(states, lists, [p for p, _, _ in layout], w)
    r, worst = 0, 0.0
    for j, (pos0, T, _) in enumerate(layout):
        z = [states[0].verify_logits(r + i) for i in range(T)]
        r += T
        for i in range(T):
            worst = max(worst, float(np.abs(z[i] - st.logits[pos0 + i]).max()))
            np.testing.assert_allclose(z[i], st.logits[pos0 + i], rtol=LOGIT_RTOL, atol=LOGIT_ATOL, err_msg=f"{name} seq {j} row {i}")
            assert int(nxts[j][i]) == np_argmax(z[i])
        assert int(accs[j]) == np_accept(lists[j], nxts[j])
        assert np.array_equal(bits(states[j].logits()), bits(z[int(accs[j])]))
        k1, v1 = caches(states[j], c)
        sl = slice(pos0, pos0 + T)
        np.testing.assert_allclose(k1[:, sl], st.k[:, sl], rtol=KV_TOL, atol=KV_TOL)
        np.testing.assert_allclose(v1[:, sl], st.v[:, sl], rtol=KV_TOL, atol=KV_TOL)
        assert not k1[:, pos0 + T:].any() and not v1[:, pos0 + T:].any()   # fresh runstates: nothing behind the call's rows
    print(f"verify_batch parity {name}: max |logit diff| {worst:.3e}")
    close_all(states, twins)


# ---- 4. neighbour invariance ---------------------------------------------------------------------------------------------------

def test_sequence_0_does_not_depend_on_its_neighbours(gpu, streams, weights):
    st, w = streams["long_gqa"], weights["long_gqa"]
    c = st.cfg
    layout = layouts(c.seq_len)["c_4x4"]
    layout = layout[2:] + layout[:2]   # sequence 0 at position 64: its neighbours are deeper and shallower
    pos0s = [p for p, _, _ in layout]
    rng = np.random.default_rng(9)

    def run(disturb):
        states, twins, lists, _ = build(gpu, st, w, layout, by_verify=False, rng=np.random.default_rng(10))
        if disturb:
            # other histories, so other cache contents everywhere the neighbours read (the API has no way to plant values in a
            # cache but to compute them), and other rows
            for j in range(1, 4):
                other = (rng.integers(2, c.vocab_size, size=pos0s[j] + 4)).astype(np.int32)
                states[j].prefill(other, 0, w)
                lists[j] = rng.integers(2, c.vocab_size, size=len(lists[j])).astype(np.int32)
        nxts, accs = gpu.verify_batch(states, lists, pos0s, w)
        out = [nxts[0].tolist(), int(accs[0]), bits(states[0].logits()).copy()]
        out += [bits(states[0].verify_logits(i)).copy() for i in range(len(lists[0]))]
        out += [bits(x).copy() for x in caches(states[0], c)]
        close_all(states, twins)
        return out

    for x, y in zip(run(False), run(True)):
        assert np.array_equal(np.asarray(x), np.asarray(y))


# ---- 5. refusals change nothing ------------------------------------------------------------------------------------------------

def test_verify_batch_contract_violations_change_nothing(gpu, ck):
    c = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    c2 = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=16)
    odd = ck.Config(dim=64, hidden_dim=174, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    w, w2, w_odd = gpu.Weights(c, None, False, seed=4), gpu.Weights(c2, None, False, seed=4), gpu.Weights(odd, None, False, seed=4)
    ss = [gpu.RunState(c) for _ in range(3)]
    s_other, odd_ss = gpu.RunState(c2), [gpu.RunState(odd) for _ in range(2)]
    comm = gpu.Comm(0, 2, None, 0, emulated=True)
    shard = gpu.RunState(c, comm)
    for j, s in enumerate(ss):
        s.prefill(np.array([3, 4 + j, 5], np.int32), 0, w)
    gpu.verify_batch(ss, [[6, 7], [8], [9, 10, 11]], 3, w, 1.0, 0.9, [[0.1, 0.2], [0.3], [0.4, 0.5, 0.6]])   # the scratch exists

    def snap():
        return [np.concatenate([x.ravel() for x in caches(s, c)] + [s.logits()]).view(np.uint32) for s in ss] + \
               [bits(ss[0].verify_logits(r)).copy() for r in range(6)]
    before = snap()
    L = gpu.lib()
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    cfg_c = ss[0].cfg
    cfg_2 = gpu.L2ZConfig(*[int(v) for v in c2.as_i32()])
    out, acc = (C.c_int32 * 32)(), (C.c_int32 * 16)()
    NULL, KEEP = "null", "keep"

    def i32(v):
        return None if v is NULL else np.array(v, np.int32).ctypes.data_as(i32p)

    def f32(v):
        return None if v is None else np.array(v, np.float32).ctypes.data_as(fp)

    def call(n=2, tokens=(1, 2, 3), n_tokens=(2, 1), pos0=(5, 5), temperature=None, top_p=None, coins=None, cfg=cfg_c,
             states=KEEP, weights=w, o=out, a=acc):
        if states is KEEP:
            states = ss[:2]
        arr = None if states is NULL else (C.c_void_p * max(len(states), 1))(*[s.h if s is not None else None for s in states])
        return L.l2z_verify_batch(n, i32(tokens), i32(n_tokens), i32(pos0), f32(temperature), f32(top_p), f32(coins),
                                  C.byref(cfg) if cfg is not None else None, arr, weights.h if weights is not None else None, o, a)

    INV, STA = gpu.ERR_INVALID, gpu.ERR_STATE
    cases = [
        (dict(tokens=NULL), INV, "null tokens"), (dict(n_tokens=NULL), INV, "null n_tokens"), (dict(pos0=NULL), INV, "null pos0"),
        (dict(cfg=None), INV, "null config"), (dict(states=NULL), INV, "null states"), (dict(states=[ss[0], None]), INV, "null runstate"),
        (dict(weights=None), INV, "null weights"), (dict(o=None), INV, "null out_next"), (dict(a=None), INV, "null out_accepted"),
        (dict(n=0), INV, "n = 0"), (dict(n=17, n_tokens=[1] * 17, pos0=[0] * 17, tokens=[1] * 17, states=ss + [ss[0]] * 14), INV, "n = 17"),
        (dict(n_tokens=(2, 0)), INV, "n_tokens[j] = 0"), (dict(n_tokens=(2, -1)), INV, "n_tokens[j] < 0"),
        (dict(tokens=[1] * 17, n_tokens=(9, 8)), INV, "17 rows"), (dict(tokens=[1] * 17, n_tokens=(17, 1)), INV, "one sequence of 17 rows"),
        (dict(states=[ss[0], ss[0]]), INV, "the same runstate twice"), (dict(states=[ss[0], shard]), INV, "a shard"),
        (dict(states=[shard, ss[0]]), INV, "a shard first"), (dict(states=[ss[0], s_other]), INV, "runstates of two configs"),
        (dict(cfg=cfg_2), INV, "another config"), (dict(weights=w2), INV, "weights of another config"),
        (dict(cfg=odd_ss[0].cfg, states=odd_ss, weights=w_odd), INV, "dims not multiples of 4"),
        (dict(temperature=(1.0, float("nan")), top_p=(0.9, 0.9), coins=(0.1, 0.2, 0.3)), INV, "temperature nan"),
        (dict(temperature=(1.0, float("inf")), top_p=(0.9, 0.9), coins=(0.1, 0.2, 0.3)), INV, "temperature inf"),
        (dict(temperature=(-0.5, 1.0), top_p=(0.9, 0.9), coins=(0.1, 0.2, 0.3)), INV, "temperature < 0"),
        (dict(temperature=(0.0, 0.0), top_p=(0.9, 1.5)), INV, "top_p > 1"),
        (dict(temperature=(1.0, 1.0), top_p=(-0.1, 0.9), coins=(0.1, 0.2, 0.3)), INV, "top_p < 0"),
        (dict(temperature=(1.0, 1.0), top_p=None, coins=(0.1, 0.2, 0.3)), INV, "top_p NULL beside temperature"),
        (dict(temperature=(0.0, 1.0), top_p=(0.9, 0.9), coins=None), INV, "coins NULL at a temperature > 0"),
        (dict(temperature=(0.0, 1.0), top_p=(0.9, 0.9), coins=(0.1, 0.2, 1.0)), INV, "coin = 1"),
        (dict(temperature=(1.0, 0.0), top_p=(0.9, 0.9), coins=(0.1, -0.2, 0.3)), INV, "coin < 0"),
        (dict(pos0=(5, -1)), STA, "pos0 < 0"), (dict(pos0=(31, 5)), STA, "pos0 + n > seq_len"), (dict(pos0=(5, 32)), STA, "pos0 = seq_len"),
        (dict(tokens=(1, -1, 3)), STA, "token < 0"), (dict(tokens=(1, 2, 512)), STA, "token = vocab"),
    ]
    for kw, code, what in cases:
        assert call(**kw) == code, what
    for b0, b1 in zip(before, snap()):
        assert np.array_equal(b0, b1)
    # what the rules let through: the last positions; a coin outside [0, 1) where the temperature is 0 (it is not read)
    assert call(pos0=(30, 31)) == gpu.OK
    assert call(temperature=(1.0, 0.0), top_p=(0.9, 0.9), coins=(0.1, 0.2, 7.0), pos0=(5, 5)) == gpu.OK
    close_all(ss, [s_other, shard], odd_ss)
    comm.close()
    for x in (w, w2, w_odd):
        x.close()


# ---- 6. the loop -----------------------------------------------------------------------------------------------------------------

PROMPTS = ([9, 400, 77, 2001, 15], [10, 5], [11, 31999, 2, 640, 3, 88, 1200], [12])   # (first ids differ: the drafter's key)
STEPS = 40


def replaying_drafter(fulls, vocab):
    """replays each sequence's known continuation (found by the history's first prompt token), every third call with
    its guesses wrong from some place on"""
    count = [0]

    def draft(hist, k):
        full = fulls[int(hist[1])]
        g = np.array(full[len(hist):len(hist) + k], np.int32)
        count[0] += 1
        j = count[0] % 5
        if count[0] % 3 == 0 and j < len(g):
            g[j:] = (g[j:] - 2 + 1) % (vocab - 2) + 2
        return g
    return draft


def check_batch_stats(toks, stats):
    assert stats["accepted"] <= stats["offered"]
    assert stats["emitted"] == sum(len(t) - len(p) - 1 for t, p in zip(toks, PROMPTS))
    assert stats["calls"] == len(stats["rows_per_call"]) and stats["rows"] == sum(stats["rows_per_call"])
    assert all(1 <= r <= 16 for r in stats["rows_per_call"])


def test_speculate_batch_emits_what_the_single_sequence_loops_emit(gpu, ck):
    cfg = ck.STORIES15M
    w = gpu.Weights(cfg, None, True, seed=15)
    temps, tops = [1.0, 0.7, 0.0, 1.0], [0.9, 1.0, 0.5, 0.0]
    coins = [gpu.coin_stream(200 + j, STEPS) for j in range(4)]

    def fresh():
        return [gpu.RunState(cfg) for _ in PROMPTS]

    base_g, base_s = [], []
    for j, p in enumerate(PROMPTS):
        ss = fresh()[:2]
        base_g.append(gpu.speculate_greedy(ss[0], w, p, STEPS, 0)[0])
        base_s.append(gpu.speculate_sample(ss[1], w, p, STEPS, 0, temps[j], tops[j], coins[j])[0])
        close_all(ss)
    for k in (0, 3, 7):
        for base, kw in ((base_g, {}), (base_s, dict(temperature=temps, top_p=tops, coins=coins))):
            fulls = {p[0]: [1] + b.tolist() for p, b in zip(PROMPTS, base)}
            ss = fresh()
            toks, stats = gpu.speculate_batch(ss, w, PROMPTS, STEPS, k, replaying_drafter(fulls, cfg.vocab_size),
                                              batched_prefill=False, **kw)
            for j in range(4):
                assert toks[j].tolist() == base[j].tolist(), (k, j, bool(kw))
            check_batch_stats(toks, stats)
            assert max(stats["rows_per_call"]) <= 4 * (k + 1)
            if k == 0:
                assert stats["offered"] == 0
            else:
                assert 0 < stats["accepted"] < stats["offered"]
            print(f"speculate_batch k={k} sampled={bool(kw)}: {stats}")
            close_all(ss)
    w.close()


def test_speculate_batch_with_the_batched_prefill_equals_the_loop_on_twins(gpu, ck):
    cfg = ck.STORIES15M
    w = gpu.Weights(cfg, None, True, seed=15)
    ss, twins = [gpu.RunState(cfg) for _ in PROMPTS], [gpu.RunState(cfg) for _ in PROMPTS]
    toks, stats = gpu.speculate_batch(ss, w, PROMPTS, STEPS, 3, batched_prefill=True)
    # the same prefill_batch call on the twins, then one-row verify calls
    hists = [[1] + list(p) for p in PROMPTS]
    gpu.prefill_batch(twins, [np.array(h, np.int32) for h in hists], 0, w)
    for j, t in enumerate(gpu.argmax_batch(twins)):
        hists[j].append(int(t))
    for j, s in enumerate(twins):
        while hists[j][-1] != 1 and len(hists[j]) - 1 < STEPS:
            nxt, a = s.verify([hists[j][-1]], len(hists[j]) - 1, w)
            assert a == 0
            hists[j].append(int(nxt[0]))
        assert toks[j].tolist() == hists[j][1:], j
        assert np.array_equal(bits(ss[j].logits()), bits(s.logits())) or 1 in hists[j][1:]
    check_batch_stats(toks, stats)
    close_all(ss, twins)
    w.close()
