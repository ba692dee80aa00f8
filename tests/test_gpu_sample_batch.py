"""l2z_sample_batch and l2z_runstate_fork on the GPU.

The sampler's token must be the host sampler's (llama2.zig_amd/host, main.zig:728-798) applied to l2z_probs_read's
probabilities with the same number, with no tolerance: the device reproduces the softmax bits, the candidates' order and
the sequential f32 sums.  The distributions are the logits of synthetic models (near uniform) and exact ones placed
with the test hook l2z_logits_write (uniform, peaked, one-hot, exact ties straddling the top-p cut).  A row's token
must not depend on the batch it is drawn in, and the call must leave the logits alone.  The fork must copy exactly the
rows it names and the logits, and a batched step after it must equal one on runstates that ran the prompt themselves.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "llama2.zig_amd", "host")
TEMPS = (0.0, 0.5, 1.0, 1.7)
TOPS = (0.0, 0.5, 0.9, 0.99, 1.0)
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


@pytest.fixture(scope="module")
def H(B):
    L = C.CDLL(os.path.join(HOST, "libllama2_host.so"))
    fp = C.POINTER(C.c_float)
    L.l2zh_sample_coin.restype = C.c_size_t
    L.l2zh_sample_coin.argtypes = [fp, C.c_size_t, C.c_float]
    L.l2zh_sample_top_p_coin.restype = C.c_size_t
    L.l2zh_sample_top_p_coin.argtypes = [fp, C.c_size_t, C.c_float, C.c_float, fp]
    L.l2zh_prng_floats.argtypes = [C.c_uint64, fp, C.c_size_t]
    return L


def host_token(H, probs, top_p, coin):
    pp = probs.ctypes.data_as(C.POINTER(C.c_float))
    if top_p in (0.0, 1.0):
        return int(H.l2zh_sample_coin(pp, probs.size, C.c_float(coin)))
    return int(H.l2zh_sample_top_p_coin(pp, probs.size, C.c_float(top_p), C.c_float(coin), None))


def coin_stream(H, seed, n):
    out = (C.c_float * n)()
    H.l2zh_prng_floats(seed, out, n)
    return [float(v) for v in out]


def model_cfg(ck, vocab):
    if vocab == 32000:
        return ck.Config(dim=288, hidden_dim=768, n_layers=2, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=64)
    return ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=vocab, seq_len=64)


def distributions(gpu, cfg, w, rng):
    """name -> logits: two synthetic-model rows (near uniform), and the hook's exact cases"""
    V = cfg.vocab_size
    s = gpu.RunState(cfg)
    out = {}
    for k, (tok, pos) in enumerate(((1, 0), (int(rng.integers(2, V)), 1))):
        s.transformer(tok, pos, w)
        out[f"model{k}"] = s.logits()
    s.close()
    out["peaked"] = out["model0"] * np.float32(20.0)
    out["uniform"] = np.zeros(V, np.float32)
    one = np.full(V, -np.inf, np.float32)
    one[int(rng.integers(0, V))] = 0.0
    out["one-hot"] = one
    # 12 tokens at scattered ids with one equal logit, far above the rest: each holds ~1/12 of the mass, so every cut
    # p in (0, 1) falls inside the tied group -- the token order among equal probabilities decides the nucleus
    ties = rng.uniform(-30.0, -20.0, V).astype(np.float32)
    ties[rng.choice(V, 12, replace=False)] = 5.0
    out["ties"] = ties
    # the tied group at a level where the cut p = 0.9 straddles it: a leader holding ~0.85, then 40 equal tokens
    strad = rng.uniform(-30.0, -20.0, V).astype(np.float32)
    ids = rng.choice(V, 41, replace=False)
    strad[ids[0]] = 4.0
    strad[ids[1:]] = np.float32(4.0 + np.log(0.15 / 0.85 / 40))
    out["straddle"] = strad
    return out


@pytest.mark.parametrize("vocab", [512, 1000, 32000])
def test_sample_batch_equals_the_host_sampler(gpu, ck, H, vocab):
    cfg = model_cfg(ck, vocab)
    w = gpu.Weights(cfg, None, vocab == 32000, seed=40 + vocab)
    rng = np.random.default_rng(vocab)
    dists = distributions(gpu, cfg, w, rng)
    states = [gpu.RunState(cfg) for _ in range(16)]
    coins = [0.0, BELOW_ONE] + coin_stream(H, vocab, 400)
    checked = 0
    for name, lg in dists.items():
        for s in states:
            s.write_logits(lg)
        for temp in TEMPS:
            probs = states[0].probs(temp) if temp > 0 else None
            want_argmax = states[0].argmax()
            for top_p in TOPS:
                # temperature 0: the coin is not used -- a few; otherwise a window of the stream (both ends included)
                k = 16 if temp == 0 else (48 if name.startswith("model") else 32)
                start = (checked * 7) % (len(coins) - k)
                cs = coins[:2] + coins[2 + start: 2 + start + k - 2]
                for c0 in range(0, k, 16):
                    chunk = cs[c0:c0 + 16]
                    got = gpu.sample_batch(states[:len(chunk)], temp, top_p, chunk)
                    for j, coin in enumerate(chunk):
                        want = want_argmax if temp == 0 else host_token(H, probs, top_p, coin)
                        assert got[j] == want, (name, temp, top_p, coin, int(got[j]), want)
                        checked += 1
    print(f"vocab {vocab}: {checked} draws identical to the host sampler")
    for s in states:
        s.close()
    w.close()


def test_sample_batch_is_batch_invariant_and_leaves_the_logits(gpu, ck, H):
    cfg = model_cfg(ck, 32000)
    w = gpu.Weights(cfg, None, True, seed=7)
    rng = np.random.default_rng(5)
    dists = list(distributions(gpu, cfg, w, rng).values())
    states = [gpu.RunState(cfg) for _ in range(16)]
    temps = [TEMPS[i % 4] for i in range(16)]
    tops = [TOPS[(i // 4 + i) % 5] for i in range(16)]
    coins = coin_stream(H, 99, 16)
    before = []
    for i, s in enumerate(states):
        s.write_logits(dists[i % len(dists)])
        before.append(s.logits())
    full = gpu.sample_batch(states, temps, tops, coins)
    for i, s in enumerate(states):
        assert gpu.sample_batch([s], temps[i], tops[i], coins[i])[0] == full[i]
        assert np.array_equal(s.logits().view(np.uint32), before[i].view(np.uint32))
    for trial in range(4):
        idx = rng.permutation(16)[:7] if trial < 2 else rng.permutation(16)
        got = gpu.sample_batch([states[i] for i in idx], [temps[i] for i in idx], [tops[i] for i in idx],
                               [coins[i] for i in idx])
        assert np.array_equal(got, full[idx]), trial
    for i, s in enumerate(states):
        assert np.array_equal(s.logits().view(np.uint32), before[i].view(np.uint32))
        s.close()
    w.close()


def test_sample_batch_contract(gpu, ck):
    cfg = model_cfg(ck, 512)
    other = model_cfg(ck, 1000)
    states = [gpu.RunState(cfg) for _ in range(17)]
    odd = gpu.RunState(other)
    lg = np.linspace(-1.0, 1.0, 512, dtype=np.float32)
    for s in states:
        s.write_logits(lg)
    nan, inf = float("nan"), float("inf")
    bad = [
        (states[:0], 1.0, 0.9, 0.5),
        (states[:17], 1.0, 0.9, 0.5),
        ([states[0], states[1], states[0]], 1.0, 0.9, 0.5),
        ([states[0], odd], 1.0, 0.9, 0.5),
        (states[:2], -1.0, 0.9, 0.5),
        (states[:2], nan, 0.9, 0.5),
        (states[:2], inf, 0.9, 0.5),
        (states[:2], 1.0, -0.1, 0.5),
        (states[:2], 1.0, 1.5, 0.5),
        (states[:2], 1.0, nan, 0.5),
        (states[:2], 1.0, 0.9, 1.0),
        (states[:2], 1.0, 0.9, -0.25),
        (states[:2], 1.0, 0.9, nan),
    ]
    for k, (ss, t, p, c) in enumerate(bad):
        with pytest.raises(gpu.L2ZError) as e:
            gpu.sample_batch(ss, t, p, c)
        assert e.value.code == gpu.ERR_INVALID, k
    L = gpu.lib()
    ss = (C.c_void_p * 2)(states[0].h, None)
    f = (C.c_float * 2)(1.0, 1.0)
    out = (C.c_int32 * 2)(-7, -7)
    assert L.l2z_sample_batch(2, ss, f, f, f, out) == gpu.ERR_INVALID
    ss = (C.c_void_p * 1)(states[0].h)
    assert L.l2z_sample_batch(1, ss, None, f, f, out) == gpu.ERR_INVALID
    assert L.l2z_sample_batch(1, ss, f, f, f, None) == gpu.ERR_INVALID
    assert list(out) == [-7, -7]
    for s in states:
        assert np.array_equal(s.logits().view(np.uint32), lg.view(np.uint32))
    # and the states still work
    assert gpu.sample_batch(states[:3], 0.0, 0.9, 0.5).tolist() == [511] * 3
    for s in states + [odd]:
        s.close()


def caches(s, c):
    kvd = c.dim // c.n_heads * c.n_kv_heads
    n = c.n_layers * c.seq_len * kvd
    return [s.read(name, 0, n).reshape(c.n_layers, c.seq_len, kvd) for name in ("key_cache", "value_cache")]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n_pos", [0, 1, 13, 64])
def test_fork_copies_the_named_rows_and_the_logits(gpu, ck, n_pos):
    cfg = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=64)
    w = gpu.Weights(cfg, None, False, seed=3)
    rng = np.random.default_rng(n_pos)
    src, dst = gpu.RunState(cfg), gpu.RunState(cfg)
    src.prefill(rng.integers(2, 512, 64).astype(np.int32), 0, w)
    dst.prefill(rng.integers(2, 512, 64).astype(np.int32), 0, w)
    dst.transformer(5, 63, w)
    sk, sv = caches(src, cfg)
    dk, dv = caches(dst, cfg)
    assert not np.array_equal(bits(sk[:, 1:]), bits(dk[:, 1:]))
    gpu.runstate_fork(dst, src, n_pos)
    k, v = caches(dst, cfg)
    for got, s_, d_ in ((k, sk, dk), (v, sv, dv)):
        assert np.array_equal(bits(got[:, :n_pos]), bits(s_[:, :n_pos]))
        assert np.array_equal(bits(got[:, n_pos:]), bits(d_[:, n_pos:]))
    assert np.array_equal(bits(dst.logits()), bits(src.logits()))
    assert dst.argmax() == src.argmax()
    k2, v2 = caches(src, cfg)
    assert np.array_equal(bits(k2), bits(sk)) and np.array_equal(bits(v2), bits(sv))
    src.close(), dst.close(), w.close()


def test_fork_contract(gpu, ck):
    cfg = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=64)
    other = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    w = gpu.Weights(cfg, None, False, seed=4)
    src, dst, odd = gpu.RunState(cfg), gpu.RunState(cfg), gpu.RunState(other)
    src.prefill(np.arange(2, 20, dtype=np.int32), 0, w)
    dst.prefill(np.arange(30, 50, dtype=np.int32), 0, w)
    before = caches(dst, cfg) + [dst.logits()]
    for n_pos in (-1, 65, 1 << 20):
        with pytest.raises(gpu.L2ZError) as e:
            gpu.runstate_fork(dst, src, n_pos)
        assert e.value.code == gpu.ERR_STATE
    for a, b in ((dst, dst), (dst, odd), (odd, src)):
        with pytest.raises(gpu.L2ZError) as e:
            gpu.runstate_fork(a, b, 4)
        assert e.value.code == gpu.ERR_INVALID
    L = gpu.lib()
    assert L.l2z_runstate_fork(None, src.h, 4) == gpu.ERR_INVALID
    assert L.l2z_runstate_fork(dst.h, None, 4) == gpu.ERR_INVALID
    after = caches(dst, cfg) + [dst.logits()]
    for x, y in zip(before, after):
        assert np.array_equal(bits(x), bits(y))
    src.close(), dst.close(), odd.close(), w.close()


@pytest.mark.parametrize("vocab", [512, 32000])
def test_batched_step_after_fork_equals_runstates_that_ran_the_prompt(gpu, ck, vocab):
    cfg = model_cfg(ck, vocab)
    w = gpu.Weights(cfg, None, vocab == 32000, seed=11)
    rng = np.random.default_rng(9)
    prompt = rng.integers(2, vocab, 23).astype(np.int32)
    n = 5
    forked = [gpu.RunState(cfg) for _ in range(n)]
    forked[0].prefill(prompt, 0, w)
    for s in forked[1:]:
        s.transformer(3, 0, w)  # something in the rows the fork leaves (and in the logits it replaces)
        gpu.runstate_fork(s, forked[0], len(prompt))
    own = [gpu.RunState(cfg) for _ in range(n)]
    for s in own:
        s.prefill(prompt, 0, w)
    for step in range(3):
        toks = rng.integers(2, vocab, n).astype(np.int32)
        pos = [len(prompt) + step] * n
        gpu.transformer_batch(forked, toks, pos, w)
        gpu.transformer_batch(own, toks, pos, w)
        for a, b in zip(forked, own):
            assert np.array_equal(bits(a.logits()), bits(b.logits())), step
    for a, b in zip(forked, own):
        ka, va = caches(a, cfg)
        kb, vb = caches(b, cfg)
        end = len(prompt) + 3
        assert np.array_equal(bits(ka[:, :end]), bits(kb[:, :end])) and np.array_equal(bits(va[:, :end]), bits(vb[:, :end]))
    for s in forked + own:
        s.close()
    w.close()
