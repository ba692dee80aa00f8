"""l2z_verify_sample on the GPU: l2z_verify's pass with every row DRAWN as l2z_sample_batch draws it, the accept scan over the
drawn ids, and the sampled speculative loop on top (binding.speculate_sample, `llama2 --spec-sample`).

The references: the host samplers (l2zh_sample_coin / l2zh_sample_top_p_coin) on the probabilities l2z_probs_read gives for a
row's logits -- the method of tests/test_gpu_sample_batch.py, no tolerance; l2z_verify for temperature 0 (uint32 compares);
the loop's own output under another number of guesses and another drafter for COIN INVARIANCE (uint32 compares); the CPU
oracle's stepped pass once, at the project's bar (5e-5), so that a sampled call's logits are covered too.

Models: those of tests/test_gpu_verify.py (the two golden toys, synthetic stories shapes, one 32000-token vocabulary)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOGIT_RTOL = 5e-5
LOGIT_ATOL = 5e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HOST = os.path.join(ROOT, "llama2.zig_amd", "host")
TOK = os.path.join(GOLD, "tokenizer.bin")
SEG = 64  # csrc/batch_decode.h kVerifySeg
TS = (1, 2, 3, 7, 16)
NAMES = ("toy_gqa_unshared", "toy_mha_shared", "stories15M", "stories110M", "wide4096", "long_gqa")
TEMPS = (0.5, 1.0, 1.7)
TOP_PS = (0.0, 0.5, 0.9, 0.99, 1.0)
COIN_LAST = float(np.nextafter(np.float32(1.0), np.float32(0.0)))


def model(ck, name):
    """(config, shared, blob)"""
    if name.startswith("toy_"):
        c, shared, blob = ck.read_checkpoint(os.path.join(GOLD, name + ".bin"))
        return c, shared, np.ascontiguousarray(blob, np.float32)
    cfg = {"stories15M": ck.STORIES15M,
           "stories110M": ck.Config(768, 2048, 12, 12, 12, 32000, 320),
           "wide4096": ck.Config(4096, 11008, 2, 32, 32, 512, 64),
           "long_gqa": ck.Config(1024, 2752, 2, 8, 4, 1024, 2048)}[name]
    return cfg, True, ck.synth_blob(cfg, True, seed=77)


@pytest.fixture(scope="module")
def H(B):
    L = C.CDLL(os.path.join(HOST, "libllama2_host.so"))
    fp = C.POINTER(C.c_float)
    L.l2zh_sample_coin.restype = C.c_size_t
    L.l2zh_sample_coin.argtypes = [fp, C.c_size_t, C.c_float]
    L.l2zh_sample_top_p_coin.restype = C.c_size_t
    L.l2zh_sample_top_p_coin.argtypes = [fp, C.c_size_t, C.c_float, C.c_float, fp]
    return L


def host_token(H, probs, top_p, coin):
    pp = probs.ctypes.data_as(C.POINTER(C.c_float))
    if top_p in (0.0, 1.0):
        return int(H.l2zh_sample_coin(pp, probs.size, C.c_float(coin)))
    return int(H.l2zh_sample_top_p_coin(pp, probs.size, C.c_float(top_p), C.c_float(coin), None))


def host_draw(H, spare, z, temperature, top_p, coin):
    """the host sampler's token for the logits z: the device's softmax(z / temperature) (l2z_probs_read), then the host walk"""
    spare.write_logits(z)
    return host_token(H, spare.probs(temperature), top_p, coin)


def caches(s, c):
    """the runstate's caches in the reference's order [layer, seq_len, kv_dim]"""
    kvd = c.dim // c.n_heads * c.n_kv_heads
    n = c.n_layers * c.seq_len * kvd
    return [s.read(name, 0, n).reshape(c.n_layers, c.seq_len, kvd) for name in ("key_cache", "value_cache")]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def np_argmax(z):
    """strict '>', lowest index"""
    return int(np.flatnonzero(z == z.max())[0])


def np_accept(tokens, nxt):
    a = 0
    while a + 1 < len(tokens) and int(tokens[a + 1]) == int(nxt[a]):
        a += 1
    return a


def wrong(t, vocab):
    """another token id, never BOS"""
    return (int(t) - 2 + 1) % (vocab - 2) + 2


def case_positions(seq_len, T):
    """0, inside a segment, up to a segment's last position, across its boundary, far out, the context's end"""
    want = [0, 17, SEG - 1, SEG - (T + 1) // 2, SEG, 5 * SEG + 220, seq_len - T]
    out = []
    for p in want:
        if 0 <= p <= seq_len - T and p not in out:
            out.append(p)
    return out


# ---- 1. every row is the host sampler's draw, exactly ---------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_the_host_samplers_draw(gpu, ck, orc, H, name):
    """Row i of a sampled call = the host sampler on probs(z_i / temperature) with coins[i], for every T, position (segment
    boundaries included), temperature, top_p, with coins of the generator's stream and with the two ends of [0, 1).  No
    tolerance.  The rows' logits against the oracle are tests/test_gpu_verify.py's business (the same pass); they are asserted
    here once, on stories15M, at the project's bar."""
    cfg, shared, blob = model(ck, name)
    V = cfg.vocab_size
    w = gpu.Weights(cfg, blob, shared)
    spare = gpu.RunState(cfg)
    rng = np.random.default_rng(2000 + NAMES.index(name))
    toks = rng.integers(2, V, size=cfg.seq_len).astype(np.int32)
    stream = gpu.coin_stream(900 + NAMES.index(name), 4096)
    ref = None
    if name == "stories15M":   # the oracle's stepped pass over the stream's first positions
        m = orc.Model(cfg.as_i32(), blob, shared)
        ref = np.stack([m.transformer(int(t), p) for p, t in enumerate(toks[:SEG + 16])])
        m.close()
    used, n_calls, n_rows, n_cmp, worst = 0, 0, 0, 0, 0.0
    for T in TS:
        for pos0 in case_positions(cfg.seq_len, T):
            s = gpu.RunState(cfg)
            if pos0:
                s.prefill(toks[:pos0], 0, w)
            rows = toks[pos0:pos0 + T]
            z, probs = None, None
            for temperature in TEMPS:
                for top_p in TOP_PS:
                    ends = np.array([(0.0, COIN_LAST)[(i + n_calls) % 2] for i in range(T)], np.float32)
                    for coins in (stream[used:used + T], ends):
                        used = (used + T) % (stream.size - 16)
                        nxt, a = s.verify_sample(rows, pos0, w, temperature, top_p, coins)
                        n_calls += 1
                        zz = [s.verify_logits(i) for i in range(T)]
                        if z is None:
                            z = zz
                            probs = {}
                            if ref is not None and pos0 + T <= ref.shape[0]:
                                for i in range(T):
                                    worst = max(worst, float(np.abs(z[i] - ref[pos0 + i]).max()))
                                    np.testing.assert_allclose(z[i], ref[pos0 + i], rtol=LOGIT_RTOL, atol=LOGIT_ATOL,
                                                               err_msg=f"{name} pos0 {pos0} T {T} row {i}")
                                    n_cmp += 1
                        else:   # the same rows at the same positions: the same bits, whatever the sampler's arguments
                            for i in range(T):
                                assert np.array_equal(bits(zz[i]), bits(z[i])), (name, pos0, T, i)
                        if temperature not in probs:
                            probs[temperature] = []
                            for i in range(T):
                                spare.write_logits(z[i])
                                probs[temperature].append(spare.probs(temperature))
                        for i in range(T):
                            want = host_token(H, probs[temperature][i], top_p, float(coins[i]))
                            assert int(nxt[i]) == want, (name, pos0, T, i, temperature, top_p, float(coins[i]))
                            n_rows += 1
                        assert a == np_accept(rows, nxt)
                        assert np.array_equal(bits(s.logits()), bits(z[a])), (name, pos0, T)
            s.close()
    if ref is not None:
        assert n_cmp > 0
        print(f"verify_sample parity {name}: {n_cmp} rows against the oracle, max |logit diff| {worst:.3e}")
    print(f"verify_sample draws {name}: {n_calls} calls, {n_rows} rows, all the host sampler's")
    spare.close(); w.close()


# ---- 2. the verdict for every accept length --------------------------------------------------------------------------------

def sampled_by_single_rows(s, w, first_token, pos0, n, temperature, top_p, coins):
    """n one-row calls from (first_token, pos0), position pos0 + i drawn with coins[i]: the tokens fed, [n + 1] (the last is
    not fed), and every position's logits row"""
    fed, rows = [int(first_token)], []
    for i in range(n):
        nxt, a = s.verify_sample([fed[-1]], pos0 + i, w, temperature, top_p, coins[i:i + 1])
        assert a == 0
        rows.append(s.verify_logits(0))
        fed.append(int(nxt[0]))
    return fed, rows


@pytest.mark.parametrize("temperature,top_p", [(1.0, 0.9), (0.7, 1.0)])
def test_sampled_verdict_for_every_accept_length(gpu, ck, H, temperature, top_p):
    cfg = ck.STORIES15M
    w = gpu.Weights(cfg, None, True, seed=3)
    spare = gpu.RunState(cfg)
    rng = np.random.default_rng(8)
    prompt = rng.integers(2, cfg.vocab_size, size=9).astype(np.int32)
    coins = gpu.coin_stream(77, 18)
    s = gpu.RunState(cfg)
    s.prefill(prompt[:8], 0, w)
    g, rows = sampled_by_single_rows(s, w, prompt[8], 8, 17, temperature, top_p, coins)   # g[0] = prompt[8], g[1 ..] drawn
    assert len(set(g[1:])) > 8   # (a sampled continuation, not one token repeated)
    for want in range(16):
        toks = np.array(g[:16], np.int32)
        if want < 15:
            toks[want + 1] = wrong(toks[want + 1], cfg.vocab_size)
            toks[want + 2:] = rng.integers(2, cfg.vocab_size, size=max(0, 16 - want - 2))
        nxt, a = s.verify_sample(toks, 8, w, temperature, top_p, coins[:16])
        assert a == np_accept(toks, nxt) == want
        assert nxt[:a + 1].tolist() == g[1:a + 2]
        za = s.verify_logits(a)
        assert np.array_equal(bits(za), bits(rows[a])), want            # (DRAFT INVARIANCE: the one-row call's bits)
        assert np.array_equal(bits(s.logits()), bits(za)), want         # the runstate's logits are row a's
        assert s.argmax() == np_argmax(za)
        for c in (0.0, 0.37, COIN_LAST):
            assert gpu.sample_batch([s], temperature, top_p, c).tolist() == [host_draw(H, spare, za, temperature, top_p, c)]
        # the next call continues the sequence: position 8 + a + 1 with its own coin
        nxt2, a2 = s.verify_sample([int(nxt[a])], 8 + a + 1, w, temperature, top_p, coins[a + 1:a + 2])
        assert a2 == 0 and int(nxt2[0]) == g[a + 2], want
        assert np.array_equal(bits(s.verify_logits(0)), bits(rows[a + 1])), want
    s.close(); spare.close(); w.close()


# ---- 3. temperature 0 is l2z_verify ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("toy_gqa_unshared", "toy_mha_shared", "stories15M", "long_gqa"))
def test_temperature_zero_is_verify_bit_for_bit(gpu, ck, name):
    cfg, shared, blob = model(ck, name)
    w = gpu.Weights(cfg, blob, shared)
    rng = np.random.default_rng(50 + NAMES.index(name))
    toks = rng.integers(2, cfg.vocab_size, size=cfg.seq_len).astype(np.int32)
    n = 0
    for T in TS:
        for pos0 in case_positions(cfg.seq_len, T):
            rows = toks[pos0:pos0 + T].copy()
            outs = []
            for how in ("verify", "null coins", "coins"):
                s = gpu.RunState(cfg)
                if pos0:
                    s.prefill(toks[:pos0], 0, w)
                if how == "verify":
                    nxt, a = s.verify(rows, pos0, w)
                    if T > 1 and n % 2 == 0:   # make the first guess right on every other case, from the model's own pick
                        rows[1] = nxt[0]
                        nxt, a = s.verify(rows, pos0, w)
                        assert a >= 1
                else:
                    coins = None if how == "null coins" else rng.random(T).astype(np.float32)
                    nxt, a = s.verify_sample(rows, pos0, w, 0.0, float(rng.choice([0.0, 0.9, 1.0])), coins)
                k, v = caches(s, cfg)
                end = pos0 + a + 1
                outs.append((nxt.tolist(), a, bits(s.logits()).copy(), [bits(s.verify_logits(i)).copy() for i in range(T)],
                             bits(k[:, :end]).copy(), bits(v[:, :end]).copy()))
                assert s.argmax() == int(nxt[a])
                s.close()
            for o in outs[1:]:
                assert o[0] == outs[0][0] and o[1] == outs[0][1], (name, pos0, T)
                assert np.array_equal(o[2], outs[0][2]), (name, pos0, T)
                for i in range(T):
                    assert np.array_equal(o[3][i], outs[0][3][i]), (name, pos0, T, i)
                assert np.array_equal(o[4], outs[0][4]) and np.array_equal(o[5], outs[0][5]), (name, pos0, T)
            n += 1
    w.close()


# ---- 4. COIN INVARIANCE ----------------------------------------------------------------------------------------------------

def check_stats(toks, stats, n_prompt):
    assert stats["accepted"] <= stats["offered"]
    assert stats["emitted"] == len(toks) - n_prompt - 1          # the first generated token is l2z_sample_batch's
    assert stats["emitted"] <= stats["accepted"] + stats["calls"]  # = sum (a + 1), cut at a BOS or the step budget


@pytest.mark.parametrize("name", ("stories15M", "long_gqa"))   # 6 heads on 6 KV heads; 8 heads on 4
@pytest.mark.parametrize("top_p", (0.9, 1.0))
def test_coin_invariance_bitwise(gpu, ck, name, top_p):
    """Fixed coins, one per generated position: the ids, the final logits and every cache row below the final position are the
    same bits for k in (0, 1, 4, 15) and for five drafters.  The drafter that is wrong with probability 1/2 cuts the calls at
    places of its own choosing: an implementation that hands coins out per call or per row, not per position, fails there."""
    cfg, shared, blob = model(ck, name)
    V = cfg.vocab_size
    w = gpu.Weights(cfg, blob, shared)
    prompt = [9, 400, 77, 201, 15]
    steps = 100   # 94 generated positions, across the segment boundary at 64
    temperature = 1.0

    def run(k, drafter, coins):
        s = gpu.RunState(cfg)
        toks, stats = gpu.speculate_sample(s, w, prompt, steps, k, temperature, top_p, coins, drafter)
        kc, vc = caches(s, cfg)
        out = (toks, stats, bits(s.logits()).copy(), bits(kc[:, :steps]).copy(), bits(vc[:, :steps]).copy())
        s.close()
        check_stats(toks, stats, len(prompt))
        return out

    for seed in range(11, 19):   # (coins under which the model does not draw BOS inside the run: the first seed, most likely)
        coins = gpu.coin_stream(seed, steps)
        base, st0, lg0, k0, v0 = run(0, None, coins)
        if 1 not in base.tolist():
            break
    assert 1 not in base.tolist() and len(base) == steps
    assert st0["offered"] == 0 and st0["calls"] == st0["emitted"] == steps - len(prompt) - 1
    assert len(set(base[len(prompt):].tolist())) > 40   # (sampled text, not a fixed point)
    full = np.concatenate([[1], base]).astype(np.int32)   # history as the drafter sees it

    def replay(hist, k):
        return full[len(hist):len(hist) + k]

    def always_wrong(hist, k):
        return np.array([wrong(t, V) for t in full[len(hist):len(hist) + k]], np.int32)

    def half_wrong_drafter():
        own = np.random.default_rng(4242)

        def d(hist, k):
            g = full[len(hist):len(hist) + k].copy()
            for i in range(len(g)):
                if own.random() < 0.5:
                    g[i] = wrong(g[i], V)
            return g
        return d

    def fewer(hist, k):
        return full[len(hist):len(hist) + max(0, k - 2)]

    n = 0
    for k in (0, 1, 4, 15):
        for what, mk in (("lookup", lambda: None), ("replay", lambda: replay), ("always wrong", lambda: always_wrong),
                         ("half wrong", half_wrong_drafter), ("fewer than k", lambda: fewer)):
            toks, stats, lg, kk, vv = run(k, mk(), coins)
            assert toks.tolist() == base.tolist(), (what, k)
            assert np.array_equal(lg, lg0), (what, k, "final logits")
            assert np.array_equal(kk, k0) and np.array_equal(vv, v0), (what, k, "cache rows")
            if k == 0:
                assert stats["offered"] == 0
            elif what == "replay":
                assert stats["accepted"] == stats["offered"] > 0
                assert stats["calls"] <= (steps - len(prompt) - 1 + k) // (k + 1) + 1
            elif what == "always wrong":
                assert stats["accepted"] == 0 and stats["offered"] > 0
            elif what == "half wrong" and k >= 4:
                # both kinds of verdict, mid-call: else the case passes vacuously
                assert 0 < stats["accepted"] < stats["offered"], stats
                assert stats["calls"] < st0["calls"]
            elif what == "fewer than k" and k >= 4:
                assert stats["accepted"] == stats["offered"] > 0
            n += 1
    # other coins, another text: the coins are what the text depends on
    other, _, _, _, _ = run(4, replay, gpu.coin_stream(seed + 100, steps))
    assert other.tolist() != base.tolist()
    print(f"coin invariance {name} top_p {top_p}: {n} runs of {steps} positions identical (coins of seed {seed})")
    w.close()


def test_speculate_sample_first_token_and_coin_indexing(gpu, ck, H):
    """coins[g] draws generated token g: restated with one-row calls and the host sampler, on the loop's own logits"""
    cfg = ck.STORIES15M
    w = gpu.Weights(cfg, None, True, seed=15)
    spare = gpu.RunState(cfg)
    prompt = [9, 400, 77]
    coins = gpu.coin_stream(5, 12)
    s = gpu.RunState(cfg)
    toks, _ = gpu.speculate_sample(s, w, prompt, 3 + 12, 4, 0.8, 0.9, coins)
    s.close()
    assert toks[:3].tolist() == prompt and len(toks) == 15
    s = gpu.RunState(cfg)
    s.prefill(np.array([1] + prompt, np.int32), 0, w)
    assert int(toks[3]) == host_draw(H, spare, s.logits(), 0.8, 0.9, float(coins[0]))
    for g in range(1, 12):
        s.verify_sample([int(toks[2 + g])], 3 + g, w, 0.8, 0.9, coins[g:g + 1])
        assert int(toks[3 + g]) == host_draw(H, spare, s.logits(), 0.8, 0.9, float(coins[g])), g
    s.close(); spare.close(); w.close()


# ---- 5. the loop ends ------------------------------------------------------------------------------------------------------

BOS_TEMPERATURE = 0.05   # the scaled BOS row's logit leads by far more than this where it is positive: drawn nearly always


def test_speculate_sample_stops_after_a_bos_inside_an_accepted_run(gpu, ck):
    """The device of test_speculate_greedy_stops_after_a_bos_inside_an_accepted_run: the classifier's BOS row is a scaled copy
    of another row, and at a low temperature the sampler draws BOS at many positions.  The raw API does not stop there:
    one-row calls give the continuation through it, a drafter that replays that continuation is always right, and the loop
    must still end with the BOS."""
    cfg = ck.STORIES15M
    blob = ck.synth_blob(cfg, False, seed=29)
    wcls = ck.carve(cfg, blob, False)["wcls"]
    wcls[1] = wcls[9] * np.float32(8.0)
    w = gpu.Weights(cfg, blob, False)
    rng = np.random.default_rng(17)
    done = 0
    for trial in range(12):
        prompt = [int(t) for t in rng.integers(2, cfg.vocab_size, size=4)]
        coins = gpu.coin_stream(300 + trial, cfg.seq_len)
        s = gpu.RunState(cfg)
        hist = np.array([1] + prompt, np.int32)
        s.prefill(hist, 0, w)
        first = int(gpu.sample_batch([s], BOS_TEMPERATURE, 0.9, coins[0])[0])
        g, _ = sampled_by_single_rows(s, w, first, len(hist), 40, BOS_TEMPERATURE, 0.9, coins[1:])
        s.close()
        full = np.concatenate([hist, g]).astype(np.int32)
        where = [i for i in range(len(hist), len(full)) if full[i] == 1]
        if not where or where[0] < len(hist) + 3 or where[0] > len(full) - 4:
            continue
        m = where[0]
        s = gpu.RunState(cfg)
        toks, stats = gpu.speculate_sample(s, w, prompt, 0, 15, BOS_TEMPERATURE, 0.9, coins,
                                           lambda h, k: full[len(h):len(h) + k])
        s.close()
        assert toks.tolist() == full[1:m + 1].tolist() and toks[-1] == 1
        assert stats["accepted"] == stats["offered"]
        done += stats["emitted"] < stats["accepted"] + stats["calls"]   # rows behind the BOS were accepted too, and dropped
    assert done >= 2, "no run had a BOS inside an accepted run: the case shows nothing"
    w.close()


def test_speculate_sample_stops_at_seq_len_with_a_shorter_last_call(gpu, ck):
    cfg = ck.Config(288, 768, 6, 6, 6, 32000, 64)
    w = gpu.Weights(cfg, None, True, seed=15)
    for seed in range(21, 29):   # (coins under which no BOS is drawn inside the context: the first seed, most likely)
        coins = gpu.coin_stream(seed, cfg.seq_len)
        s = gpu.RunState(cfg)
        base, _ = gpu.speculate_sample(s, w, [5, 6], 0, 0, 1.0, 0.9, coins)
        s.close()
        if 1 not in base.tolist():
            break
    assert 1 not in base.tolist() and len(base) == cfg.seq_len
    full = np.concatenate([[1], base]).astype(np.int32)
    asked = []

    def replay(hist, k):
        asked.append((len(hist), k))
        return full[len(hist):len(hist) + k]

    s = gpu.RunState(cfg)
    toks, stats = gpu.speculate_sample(s, w, [5, 6], 0, 15, 1.0, 0.9, coins, replay)
    assert toks.tolist() == base.tolist()
    for n_hist, k in asked:   # the call's rows are positions n_hist - 1 .. n_hist - 1 + k
        assert n_hist - 1 + k <= cfg.seq_len - 1
    assert 0 < asked[-1][1] < 15 and asked[-1][0] - 1 + asked[-1][1] == cfg.seq_len - 1
    with pytest.raises(ValueError):   # one coin short of the 62 generated positions
        gpu.speculate_sample(s, w, [5, 6], 0, 15, 1.0, 0.9, coins[:61], replay)
    s.close(); w.close()


# ---- 6. refusals change nothing --------------------------------------------------------------------------------------------

def test_verify_sample_contract_violations_change_nothing(gpu, ck):
    c = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    c2 = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=16)
    odd = ck.Config(dim=64, hidden_dim=174, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    w = gpu.Weights(c, None, False, seed=4)
    w_odd = gpu.Weights(odd, None, False, seed=4)
    s, twin = gpu.RunState(c), gpu.RunState(c)
    s_odd = gpu.RunState(odd)
    good = np.array([0.3, 0.8], np.float32)
    for x in (s, twin):
        x.prefill(np.array([3, 4, 5], np.int32), 0, w)
        x.verify_sample([6, 7], 3, w, 1.0, 0.9, good)   # (the scratch exists: a refusal must not touch it either)
    expected = twin.verify_sample([8, 9, 10], 4, w, 0.9, 0.9, [0.1, 0.5, 0.7])   # what the next valid call gives
    comm = gpu.Comm(0, 2, None, 0, emulated=True)
    shard = gpu.RunState(c, comm)

    def snap():
        return (np.concatenate([x.ravel() for x in caches(s, c)]).view(np.uint32), bits(s.logits()).copy(),
                bits(s.verify_logits(1)).copy())
    before = snap()
    L = gpu.lib()
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    cfg_c = s.cfg
    cfg_2 = gpu.L2ZConfig(*[int(v) for v in c2.as_i32()])
    out = (C.c_int32 * 17)()
    acc = C.c_int(0)
    nan, inf = float("nan"), float("inf")

    def call(tokens, n, pos0, t=1.0, p=0.9, coins=(0.3, 0.8), cfg=cfg_c, state=s, weights=w, o=out, a=C.byref(acc)):
        tk = np.array(tokens if tokens is not None else [0], np.int32)
        cc = np.zeros(17, np.float32)
        if coins is not None:
            cc[:len(coins)] = coins
        return L.l2z_verify_sample(tk.ctypes.data_as(i32p) if tokens is not None else None, n, pos0, C.c_float(t), C.c_float(p),
                                   cc.ctypes.data_as(fp) if coins is not None else None, C.byref(cfg),
                                   state.h if state is not None else None, weights.h if weights is not None else None, o, a)

    cases = [
        # l2z_verify's own
        (dict(tokens=None, n=1, pos0=5), gpu.ERR_INVALID, "null tokens"),
        (dict(tokens=[1], n=1, pos0=5, state=None), gpu.ERR_INVALID, "null runstate"),
        (dict(tokens=[1], n=1, pos0=5, weights=None), gpu.ERR_INVALID, "null weights"),
        (dict(tokens=[1], n=1, pos0=5, o=None), gpu.ERR_INVALID, "null out_next"),
        (dict(tokens=[1], n=1, pos0=5, a=None), gpu.ERR_INVALID, "null out_accepted"),
        (dict(tokens=[1], n=0, pos0=5), gpu.ERR_INVALID, "n = 0"),
        (dict(tokens=[1] * 17, n=17, pos0=5), gpu.ERR_INVALID, "n = 17"),
        (dict(tokens=[1, 2], n=2, pos0=5, state=shard), gpu.ERR_INVALID, "shard"),
        (dict(tokens=[1, 2], n=2, pos0=5, cfg=cfg_2), gpu.ERR_INVALID, "another config"),
        (dict(tokens=[1, 2], n=2, pos0=5, cfg=s_odd.cfg, state=s_odd, weights=w_odd), gpu.ERR_INVALID, "dims not multiples of 4"),
        (dict(tokens=[1, 2], n=2, pos0=-1), gpu.ERR_STATE, "pos0 < 0"),
        (dict(tokens=[1, 2], n=2, pos0=31), gpu.ERR_STATE, "pos0 + n > seq_len"),
        (dict(tokens=[1, 2], n=2, pos0=32), gpu.ERR_STATE, "pos0 = seq_len"),
        (dict(tokens=[1, -1], n=2, pos0=5), gpu.ERR_STATE, "token < 0"),
        (dict(tokens=[1, 512], n=2, pos0=5), gpu.ERR_STATE, "token = vocab"),
        (dict(tokens=[1, 512], n=2, pos0=5, t=0.0, coins=None), gpu.ERR_STATE, "token = vocab at temperature 0"),
        # the sampler's
        (dict(tokens=[1, 2], n=2, pos0=5, t=nan), gpu.ERR_INVALID, "temperature nan"),
        (dict(tokens=[1, 2], n=2, pos0=5, t=inf), gpu.ERR_INVALID, "temperature inf"),
        (dict(tokens=[1, 2], n=2, pos0=5, t=-0.5), gpu.ERR_INVALID, "temperature < 0"),
        (dict(tokens=[1, 2], n=2, pos0=5, p=-0.1), gpu.ERR_INVALID, "top_p < 0"),
        (dict(tokens=[1, 2], n=2, pos0=5, p=1.5), gpu.ERR_INVALID, "top_p > 1"),
        (dict(tokens=[1, 2], n=2, pos0=5, p=nan), gpu.ERR_INVALID, "top_p nan"),
        (dict(tokens=[1, 2], n=2, pos0=5, t=0.0, p=1.5, coins=None), gpu.ERR_INVALID, "top_p > 1 at temperature 0"),
        (dict(tokens=[1, 2], n=2, pos0=5, coins=None), gpu.ERR_INVALID, "null coins at a temperature"),
        (dict(tokens=[1, 2], n=2, pos0=5, coins=(0.3, 1.0)), gpu.ERR_INVALID, "coin = 1"),
        (dict(tokens=[1, 2], n=2, pos0=5, coins=(-0.1, 0.5)), gpu.ERR_INVALID, "coin < 0"),
        (dict(tokens=[1, 2], n=2, pos0=5, coins=(0.3, nan)), gpu.ERR_INVALID, "coin nan"),
    ]
    for kw, code, what in cases:
        assert call(**kw) == code, what
    with pytest.raises(gpu.L2ZError) as e:
        s.verify_logits(2)   # the last call had two rows
    assert e.value.code == gpu.ERR_STATE
    after = snap()
    for b0, b1 in zip(before, after):
        assert np.array_equal(b0, b1)
    # a coin outside the call's rows is not looked at; then the next valid call gives what it gave the twin
    assert call([1, 2], 2, 30, coins=(0.3, 0.8, 7.0)) == gpu.OK   # the last two positions are a valid call
    got = s.verify_sample([8, 9, 10], 4, w, 0.9, 0.9, [0.1, 0.5, 0.7])
    assert got[0].tolist() == expected[0].tolist() and got[1] == expected[1]
    assert np.array_equal(bits(s.logits()), bits(twin.logits()))
    for x in (s, twin, s_odd, shard):
        x.close()
    comm.close()
    w.close(); w_odd.close()


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------

def run_cli(ckpt, extra, prompt=None, n=24):
    args = [os.path.join(HOST, "llama2"), os.path.join(GOLD, ckpt), "-n", str(n), "-z", TOK, "-v", "--tokens", *extra]
    if prompt:
        args += ["-i", prompt]
    r = subprocess.run(args, capture_output=True, timeout=180)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, err
    ids = [int(t) for t in [l for l in err.splitlines() if l.startswith("tokens:")][0].split()[1:]]
    return ids, r.stdout, err


def test_cli_spec_sample_prints_the_same_text_for_every_k(gpu, ck):
    """`--spec-sample K -s SEED -t 1.0 -p 0.9` prints the same bytes for K in (0, 1, 4, 15); its ids are speculate_sample's
    under coin_stream(SEED); `-t 0 --spec-sample 4` is `-t 0 --spec 4`.

    Equality with the PLAIN sampled CLI at the same seed is not asserted: the plain loop's logits come from l2z_transformer,
    whose bits differ from a verify row's within the parity bar, and a nucleus has as many cdf boundaries as candidates, so a
    coin can land on the other side of one.  The comparison is printed."""
    seed = 1234
    for ckpt, prompt in (("toy_gqa_unshared.bin", None), ("toy_mha_shared.bin", "a b")):
        c, shared, blob = ck.read_checkpoint(os.path.join(GOLD, ckpt))
        prompt_ids = []
        if prompt:   # --score lists the prompt's ids: pos, id, piece, ...
            r = subprocess.run([os.path.join(HOST, "llama2"), os.path.join(GOLD, ckpt), "-z", TOK, "--score", "-i", prompt],
                               capture_output=True, timeout=180, check=True)
            prompt_ids = [int(l.split("\t")[1]) for l in r.stdout.decode(errors="replace").splitlines() if l.count("\t") >= 4]
            assert prompt_ids
        outs = []
        for K in (0, 1, 4, 15):
            ids, text, err = run_cli(ckpt, ["--spec-sample", str(K), "-s", str(seed), "-t", "1.0", "-p", "0.9"], prompt)
            assert "spec-sample:" in err
            outs.append((ids, text))
        for o in outs[1:]:
            assert o == outs[0], ckpt
        w, s = gpu.Weights(c, np.ascontiguousarray(blob, np.float32), shared), gpu.RunState(c)
        toks, _ = gpu.speculate_sample(s, w, prompt_ids, 24, 4, 1.0, 0.9, gpu.coin_stream(seed, 24))
        assert toks.tolist() == outs[0][0], ckpt
        s.close(); w.close()
        other, _, _ = run_cli(ckpt, ["--spec-sample", "4", "-s", str(seed + 1), "-t", "1.0", "-p", "0.9"], prompt)
        assert other != outs[0][0]   # (the seed is what the text depends on)
        plain, _, _ = run_cli(ckpt, ["-s", str(seed), "-t", "1.0", "-p", "0.9"], prompt)
        print(f"{ckpt}: plain sampled CLI at the same seed {'equals' if plain == outs[0][0] else 'differs from'} --spec-sample")
        a = run_cli(ckpt, ["-t", "0", "--spec-sample", "4"], prompt)
        b = run_cli(ckpt, ["-t", "0", "--spec", "4"], prompt)
        assert a[:2] == b[:2], ckpt


# ---- 8. it composes --------------------------------------------------------------------------------------------------------

def test_verify_sample_composes_with_the_other_entry_points(gpu, ck, orc):
    """after a sampled call that rejected guesses, each of the other entry points continues at pos0 + a + 1 and meets the oracle"""
    cfg, shared, blob = model(ck, "stories15M")
    w = gpu.Weights(cfg, blob, shared)
    rng = np.random.default_rng(1002)
    toks = rng.integers(2, cfg.vocab_size, size=64).astype(np.int32)
    m = orc.Model(cfg.as_i32(), blob, shared)
    ref = np.stack([m.transformer(int(t), p) for p, t in enumerate(toks)])
    m.close()
    pos0 = 40
    coins = gpu.coin_stream(8, 8)

    def after_call():
        s = gpu.RunState(cfg)
        s.prefill(toks[:pos0], 0, w)
        nxt, a = s.verify_sample(toks[pos0:pos0 + 8], pos0, w, 1.0, 0.9, coins)
        assert a < 7   # random guesses: rejected (rows a + 1 .. 7 are stale now)
        return s, pos0 + a + 1   # continue the STREAM: its token at pos0 + a + 1

    def close(z, p):
        np.testing.assert_allclose(z, ref[p], rtol=LOGIT_RTOL, atol=LOGIT_ATOL)

    s, p = after_call()
    assert gpu.sample_batch([s], 0.0, 0.9, 0.5).tolist() == [s.argmax()]
    s.transformer(int(toks[p]), p, w)
    close(s.logits(), p)
    s.close()

    s, p = after_call()
    comp = gpu.RunState(cfg)
    gpu.transformer_batch([comp, s], [5, int(toks[p])], [0, p], w)
    close(s.logits(), p)
    s.close(); comp.close()

    s, p = after_call()
    s.prefill(toks[p:p + 6], p, w)
    close(s.logits(), p + 5)
    s.close()

    s, p = after_call()
    dst = gpu.RunState(cfg)
    gpu.runstate_fork(dst, s, p)
    assert np.array_equal(bits(dst.logits()), bits(s.logits()))
    dst.transformer(int(toks[p]), p, w)
    close(dst.logits(), p)
    dst.verify_sample(toks[p + 1:p + 4], p + 1, w, 1.0, 0.9, coins[:3])
    close(dst.verify_logits(2), p + 3)
    dst.verify(toks[p + 4:p + 6], p + 4, w)
    close(dst.verify_logits(1), p + 5)
    s.close(); dst.close()
    w.close()
