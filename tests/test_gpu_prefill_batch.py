"""l2z_prefill_batch on the GPU: the prompts of up to 16 sequences, one runstate each, in one pass over the concatenated rows.

For every sequence the call must leave what l2z_prefill of that sequence alone leaves.  Checked against the CPU oracle's
stepped pass, per sequence: the last position's logits within THE BAR of tests/test_gpu_parity.py (LOGIT_ATOL + LOGIT_RTOL *
max |z|), then four more positions through l2z_transformer_batch fed the oracle's own argmax (they read the scattered KV
rows) at the same bar; token ids where the oracle's margin exceeds the bar; and, secondarily, within twice the bar of a plain
l2z_prefill of the same sequence on the same build.  Neighbour invariance, the cache footprint and the contract are
checked bit for bit.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_gpu_parity import LOGIT_ATOL, LOGIT_RTOL, PREFILL_CONFIGS, SHARDED_PREFILL

pytestmark = pytest.mark.gpu

SMALL = dict(dim=288, hidden_dim=768, n_layers=2, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=320)   # head size 48
GQA = dict(next(c for c in SHARDED_PREFILL if c[0] == "gqa")[1])                                             # head size 32
STREAMS = dict(next(c for c in PREFILL_CONFIGS if c[0] == "streams-2048")[1])                                # head size 128: flash form
# head size 64 with grouped kv heads: the other flash instantiation; head size 256 with one kv head: the general form at the
# widest head l2z_prefill takes (small and gqa take the general form too)
HS64 = dict(dim=512, hidden_dim=1408, n_layers=2, n_heads=8, n_kv_heads=2, vocab_size=1024, seq_len=320)
MQA256 = dict(dim=512, hidden_dim=1408, n_layers=2, n_heads=2, n_kv_heads=1, vocab_size=1024, seq_len=96)
SHAPES = {"small": SMALL, "gqa": GQA, "streams-2048": STREAMS, "hs64": HS64, "mqa-256": MQA256}
SEED = 23
N_STEPS = 4   # positions decoded after the call

# id -> (shape, shared classifier, lengths, positions the sequences start at (0: a fresh one; > 0: after l2z_prefill of a
#        common prefix + l2z_runstate_fork), L2Z_PF_X3, L2Z_PF_CHUNK)
CASES = {
    "small-one": ("small", False, [37], None, 1, 0),
    "small-16-equal": ("small", False, [20] * 16, None, 1, 0),
    "small-mixed": ("small", False, [1, 5, 33, 1, 64, 17, 2], None, 1, 0),
    "small-mixed-shared": ("small", True, [1, 5, 33, 1, 64, 17, 2], None, 1, 0),
    "small-mixed-x3": ("small", False, [1, 5, 33, 1, 64, 17, 2], None, 2, 0),
    # totals on both sides of the 16 / 32 / 128 / 129-row switch-overs of the GEMM forms
    **{f"small-total-{sum(ls)}": ("small", False, ls, None, 1, 0)
       for ls in ([7, 9], [8, 9], [15, 17], [16, 17], [60, 68], [60, 69])},
    # chunks of 64 rows: sequence 1 straddles one boundary, sequence 2 two
    "small-straddle": ("small", False, [50, 40, 70], None, 1, 64),
    "small-continued": ("small", False, [10, 20, 7, 12], [24, 24, 24, 0], 1, 0),
    "gqa-two-chunks": ("gqa", False, [70, 130, 9, 300, 21], None, 1, 0),          # 530 rows: 512 + 18
    "streams-mixed": ("streams-2048", False, [40, 3, 90, 1, 30], None, 1, 0),     # layers on the bf16 cores, flash attention
    "streams-mixed-x3": ("streams-2048", False, [40, 3, 90, 1, 30], None, 2, 0),
    "streams-straddle-continued": ("streams-2048", False, [50, 70, 1, 30], [0, 16, 16, 0], 1, 64),
    "hs64-mixed": ("hs64", False, [100, 3, 64, 65, 1], None, 1, 0),
    "hs64-shared-continued": ("hs64", True, [30, 66, 2], [20, 0, 20], 1, 0),
    "mqa-256-mixed": ("mqa-256", False, [30, 1, 50], None, 1, 0),
}


def bar_of(z):
    return LOGIT_ATOL + LOGIT_RTOL * float(np.abs(z).max())


def case_tokens(cfg, lengths, pos0s, salt=0):
    """(the common prefix, one token array per sequence); sequences of another `salt` share nothing"""
    rng = np.random.default_rng([SEED, salt, len(lengths), sum(lengths)])
    prefix = np.array([1] + rng.integers(2, cfg.vocab_size, max(pos0s) - 1).tolist(), np.int32) if max(pos0s) else np.zeros(0, np.int32)
    lists = []
    for n, p in zip(lengths, pos0s):
        t = rng.integers(2, cfg.vocab_size, n).astype(np.int32)
        if p == 0:
            t[0] = 1
        lists.append(t)
    return prefix, lists


def oracle_sequence(orc, cfg, blob, shared, history, tokens):
    """the oracle's stepped pass over history + tokens, then N_STEPS positions on its own argmax: the logits after the
    last prompt token and after every step, the tokens it fed, and (argmax, margin) of every one of those logits"""
    m = orc.Model(cfg.as_i32(), blob, shared)
    z = None
    pos = 0
    for t in list(history) + list(tokens):
        z = m.transformer(int(t), pos)
        pos += 1
    zs, fed = [z], []
    for _ in range(N_STEPS):
        t = int(np.argmax(zs[-1]))
        fed.append(t)
        zs.append(m.transformer(t, pos))
        pos += 1
    m.close()
    tops, margins = [], []
    for z in zs:
        two = np.partition(z.astype(np.float64), -2)[-2:]
        tops.append(int(np.argmax(z)))
        margins.append(float(two[1] - two[0]))
    return zs, fed, tops, margins


def make_states(gpu, cfg, w, prefix, pos0s):
    """one runstate per sequence; those that start at pos0 > 0 hold rows 0 .. pos0 - 1 of the common prefix (prefill + fork)"""
    states = [gpu.RunState(cfg) for _ in pos0s]
    if max(pos0s):
        base = gpu.RunState(cfg)
        base.prefill(prefix, 0, w)
        for s, p in zip(states, pos0s):
            if p:
                gpu.runstate_fork(s, base, p)
        for s in states:
            s.synchronize()
        base.close()
    return states


@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_the_oracle_per_sequence(gpu, ck, orc, options, case):
    shape, shared, lengths, pos0s, x3, chunk = CASES[case]
    pos0s = pos0s or [0] * len(lengths)
    options(L2Z_PF_X3=x3, L2Z_PF_CHUNK=chunk)
    cfg = ck.Config(**SHAPES[shape])
    blob = ck.synth_blob(cfg, shared, seed=SEED)
    prefix, lists = case_tokens(cfg, lengths, pos0s)
    n = len(lists)
    with ThreadPoolExecutor(8) as ex:  # the oracle's calls release the GIL
        ref = list(ex.map(lambda j: oracle_sequence(orc, cfg, blob, shared, prefix[:pos0s[j]], lists[j]), range(n)))
    w = gpu.Weights(cfg, blob, shared)
    states = make_states(gpu, cfg, w, prefix, pos0s)
    gpu.prefill_batch(states, lists, pos0s, w)
    worst, skipped, positions = 0.0, 0, 0

    def check(step):
        nonlocal worst, skipped, positions
        ids = gpu.argmax_batch(states)
        for j, s in enumerate(states):
            z = ref[j][0][step]
            bar = bar_of(z)
            err = float(np.abs(s.logits() - z).max())
            worst = max(worst, err / bar)
            print(f"prefill_batch {case}: sequence {j} step {step}: max |dlogit| {err:.3e}, bar {bar:.3e}, margin {ref[j][3][step]:.3e}")
            assert err <= bar, (case, j, step, err, bar)
            positions += 1
            if ref[j][3][step] > bar:
                assert int(ids[j]) == ref[j][2][step], (case, j, step)
            else:
                skipped += 1

    check(0)
    # secondary: a plain l2z_prefill of each sequence on the same build, each side within the bar of the oracle
    for j in (0, n // 2, n - 1):
        alone = make_states(gpu, cfg, w, prefix, [pos0s[j]])[0]
        alone.prefill(lists[j], pos0s[j], w)
        d = float(np.abs(alone.logits() - states[j].logits()).max())
        assert d <= 2 * bar_of(ref[j][0][0]), (case, j, d)
        alone.close()
    for step in range(1, N_STEPS + 1):
        gpu.transformer_batch(states, [ref[j][1][step - 1] for j in range(n)],
                              [pos0s[j] + lengths[j] + step - 1 for j in range(n)], w)
        check(step)
    print(f"prefill_batch {case}: worst error {worst:.3f} of its bar; {skipped} of {positions} positions under the margin rule")
    assert skipped <= 0.02 * positions, "vacuous: too many positions left out of the token comparison"
    for s in states:
        s.close()
    w.close()


def caches(s, c):
    """the runstate's caches in the reference's order [layer, seq_len, kv_dim] (l2z_runstate_read permutes)"""
    kvd = c.dim // c.n_heads * c.n_kv_heads
    n = c.n_layers * c.seq_len * kvd
    return [s.read(name, 0, n).reshape(c.n_layers, c.seq_len, kvd) for name in ("key_cache", "value_cache")]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def stale_states(gpu, cfg, w, n, salt):
    """runstates whose caches hold OTHER contents in every row: a prefill of the whole context with tokens of their own"""
    out = []
    for j in range(n):
        s = gpu.RunState(cfg)
        t = np.random.default_rng([salt, j]).integers(2, cfg.vocab_size, cfg.seq_len).astype(np.int32)
        s.prefill(t, 0, w)
        s.synchronize()
        out.append(s)
    return out


INVARIANCE = {
    # shape, lengths, pos0s, L2Z_PF_CHUNK
    "small-straddle": ("small", [50, 40, 70, 1, 9], [0, 0, 0, 0, 0], 64),        # general attention form, three chunks
    "streams-continued": ("streams-2048", [40, 3, 90, 1, 30], [0, 16, 0, 16, 0], 0),   # flash form, the bf16 cores
}


@pytest.mark.parametrize("name", list(INVARIANCE))
def test_neighbour_invariance_and_run_to_run(gpu, ck, options, name):
    """a fixed layout: sequence j's logits and KV rows are the same bits whatever tokens the others hold, whatever the
    others' caches contain, whatever stale rows its own cache holds beyond its range -- and from run to run"""
    shape, lengths, pos0s, chunk = INVARIANCE[name]
    options(L2Z_PF_CHUNK=chunk)
    cfg = ck.Config(**SHAPES[shape])
    w = gpu.Weights(cfg, ck.synth_blob(cfg, False, seed=SEED), False)
    prefix, lists = case_tokens(cfg, lengths, pos0s)
    _, others = case_tokens(cfg, lengths, pos0s, salt=1)
    n = len(lists)

    def rows_of(states):
        out = []
        for j, s in enumerate(states):
            k, v = caches(s, cfg)
            lo, hi = pos0s[j], pos0s[j] + lengths[j]
            out.append((bits(s.logits()), bits(k[:, lo:hi]), bits(v[:, lo:hi])))
        return out

    def run(tok_lists, stale_salt=None):
        if stale_salt is None:
            states = make_states(gpu, cfg, w, prefix, pos0s)
        else:   # every cache full of other contents, rows 0 .. pos0 - 1 of the continued ones then set by the fork
            states = stale_states(gpu, cfg, w, n, stale_salt)
            if max(pos0s):
                base = gpu.RunState(cfg)
                base.prefill(prefix, 0, w)
                for s, p in zip(states, pos0s):
                    if p:
                        gpu.runstate_fork(s, base, p)
                for s in states:
                    s.synchronize()
                base.close()
        gpu.prefill_batch(states, tok_lists, pos0s, w)
        got = rows_of(states)
        for s in states:
            s.close()
        return got

    first = run(lists)
    again = run(lists)
    for j in range(n):
        for a, b in zip(first[j], again[j]):
            assert np.array_equal(a, b), (name, "run to run", j)
    for j in range(n):
        mixed = [lists[i] if i == j else others[i] for i in range(n)]
        got = run(mixed, stale_salt=100 + j)
        for a, b in zip(first[j], got[j]):
            assert np.array_equal(a, b), (name, "neighbours", j)
    w.close()


@pytest.mark.parametrize("shape,lengths,pos0s,chunk", [("small", [50, 40, 70, 1], [3, 0, 200, 319], 64),
                                                       ("hs64", [100, 3, 65], [0, 17, 255], 0)], ids=["small", "hs64"])
def test_footprint_only_the_sequences_own_rows_are_written(gpu, ck, options, shape, lengths, pos0s, chunk):
    """every cache holds a pattern of its own in every row; after the call every row outside [pos0[j], pos0[j] + n_tokens[j])
    of every layer of every runstate holds it still, bit for bit, and a bystander runstate's too"""
    options(L2Z_PF_CHUNK=chunk)
    cfg = ck.Config(**SHAPES[shape])
    w = gpu.Weights(cfg, ck.synth_blob(cfg, False, seed=SEED), False)
    n = len(lengths)
    states = stale_states(gpu, cfg, w, n + 1, salt=7)
    before = [caches(s, cfg) for s in states]
    logits_by = bits(states[n].logits())
    _, lists = case_tokens(cfg, lengths, [0] * n)
    gpu.prefill_batch(states[:n], lists, pos0s, w)
    for j, s in enumerate(states):
        keep = np.ones(cfg.seq_len, bool)
        if j < n:
            keep[pos0s[j]:pos0s[j] + lengths[j]] = False
        for got, was in zip(caches(s, cfg), before[j]):
            assert np.array_equal(bits(got[:, keep]), bits(was[:, keep])), (j, "rows outside the range changed")
            if j < n:
                assert not np.array_equal(bits(got[:, ~keep]), bits(was[:, ~keep])), (j, "rows inside the range not written")
    assert np.array_equal(bits(states[n].logits()), logits_by)
    for s in states:
        s.close()
    w.close()


def test_contract_refusals_change_nothing(gpu, ck):
    cfg = ck.Config(**SHAPES["hs64"])
    other = ck.Config(**dict(SHAPES["hs64"], seq_len=64))
    blob = ck.synth_blob(cfg, False, seed=SEED)
    w = gpu.Weights(cfg, blob, False)
    w_other = gpu.Weights(other, ck.synth_blob(other, False, seed=SEED), False)
    states = stale_states(gpu, cfg, w, 3, salt=9)
    s_other = gpu.RunState(other)
    comm = gpu.Comm(0, 2, None, 0, emulated=True)
    s_shard = gpu.RunState(cfg, comm)
    many = [gpu.RunState(other) for _ in range(17)]
    before = [(bits(s.logits()), [bits(x) for x in caches(s, cfg)]) for s in states]
    V, S = cfg.vocab_size, cfg.seq_len
    a, b, c = states

    def refused(code, ss, lists, pos0s, weights=w):
        with pytest.raises(gpu.L2ZError) as e:
            gpu.prefill_batch(ss, lists, pos0s, weights)
        assert e.value.code == code, (e.value, lists, pos0s)

    ok = [[1, 5, 6], [1, 7]]
    refused(gpu.ERR_INVALID, [], [], [])                                      # n = 0
    refused(gpu.ERR_INVALID, many, [[1]] * 17, 0, w_other)                    # n = 17
    refused(gpu.ERR_INVALID, [a, b], [[1, 5, 6], []], 0)                      # an empty sequence
    refused(gpu.ERR_INVALID, [a, a], ok, 0)                                   # the same runstate twice
    refused(gpu.ERR_INVALID, [a, s_other], ok, 0)                             # a runstate of another config
    refused(gpu.ERR_INVALID, [a, s_shard], ok, 0)                             # a shard
    refused(gpu.ERR_INVALID, [a, b], ok, 0, w_other)                          # weights of another config
    refused(gpu.ERR_STATE, [a, b], ok, [0, -1])
    refused(gpu.ERR_STATE, [a, b], ok, [S - 2, 0])                            # 3 tokens from seq_len - 2
    refused(gpu.ERR_STATE, [a, b], [[1, 5, V], [1, 7]], 0)
    refused(gpu.ERR_STATE, [a, b], [[1, 5, 6], [-1, 7]], 0)
    # NULL arguments, straight through the C ABI
    L = gpu.lib()
    i32 = C.POINTER(C.c_int32)
    tok, nt, p0 = (C.c_int32 * 5)(1, 5, 6, 1, 7), (C.c_int32 * 2)(3, 2), (C.c_int32 * 2)(0, 0)
    ss = (C.c_void_p * 2)(a.h, b.h)
    null_i32 = C.cast(None, i32)
    good = [2, tok, nt, p0, C.byref(a.cfg), ss, w.h]
    for k in (1, 2, 3, 4, 5, 6):
        args = list(good)
        args[k] = null_i32 if k in (1, 2, 3) else None
        assert L.l2z_prefill_batch(*args) == gpu.ERR_INVALID, k
    ss_null = (C.c_void_p * 2)(a.h, None)
    assert L.l2z_prefill_batch(2, tok, nt, p0, C.byref(a.cfg), ss_null, w.h) == gpu.ERR_INVALID
    # dims l2z_prefill refuses: a head size that is not a multiple of 4
    odd = ck.Config(dim=36, hidden_dim=96, n_layers=1, n_heads=6, n_kv_heads=6, vocab_size=64, seq_len=16)
    w_odd, s_odd = gpu.Weights(odd, ck.synth_blob(odd, False, seed=SEED), False), gpu.RunState(odd)
    with pytest.raises(gpu.L2ZError) as e:
        s_odd.prefill([1, 2], 0, w_odd)
    assert e.value.code == gpu.ERR_INVALID
    refused(gpu.ERR_INVALID, [s_odd], [[1, 2]], 0, w_odd)
    for s, (lg, kv) in zip(states, before):
        assert np.array_equal(bits(s.logits()), lg)
        for got, was in zip(caches(s, cfg), kv):
            assert np.array_equal(bits(got), was)
    # ... and the same arguments are accepted once they are right
    gpu.prefill_batch([a, b], ok, 0, w)
    assert not np.array_equal(bits(a.logits()), before[0][0])
    for s in states + [s_other, s_shard, s_odd] + many:
        s.close()
    comm.close()
    for x in (w, w_other, w_odd):
        x.close()
