"""l2z_verify on the GPU: several consecutive positions of ONE sequence in one sweep of the weights, the verdict on the
guesses among them, and the speculative greedy loop on top (binding.speculate_greedy, `llama2 --spec`).

The references: the CPU oracle's stepped pass for values (logits rtol = atol = 5e-5, KV rows 2e-5: the bars of
tests/test_gpu_batch_decode.py), a numpy restatement of the argmax / accept rule for the verdict, and the call's own bits
under another cut of the same positions for DRAFT INVARIANCE (uint32 compares).

Every model gets ONE random token stream as long as its context and ONE oracle pass over it.  A case (pos0, T) feeds
stream[:pos0] as history and stream[pos0 : pos0 + T] as the call's rows: the guesses are random, so nearly all are wrong,
and row i's logits are still the oracle's at position pos0 + i of the stream.

The two golden toy models have contexts of 32 and 24 positions: where a case needs 48 positions they run their whole
context, cut the same way."""
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LOGIT_RTOL = 5e-5
LOGIT_ATOL = 5e-5
KV_TOL = 2e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HOST = os.path.join(ROOT, "llama2.zig_amd", "host")
TOK = os.path.join(GOLD, "tokenizer.bin")
SEG = 64  # csrc/batch_decode.h kVerifySeg: the attention's segments are SEG absolute positions each
TS = (1, 2, 3, 7, 16)
NAMES = ("toy_gqa_unshared", "toy_mha_shared", "stories15M", "stories110M", "wide4096", "long_gqa")


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


class Stream:
    """a model, its random stream over the whole context and the oracle's stepped pass over it"""

    def __init__(self, ck, orc, name):
        self.name = name
        self.cfg, self.shared, self.blob = model(ck, name)
        c = self.cfg
        rng = np.random.default_rng(1000 + NAMES.index(name))
        self.toks = rng.integers(2, c.vocab_size, size=c.seq_len).astype(np.int32)
        m = orc.Model(c.as_i32(), self.blob, self.shared)
        self.logits = np.empty((c.seq_len, c.vocab_size), np.float32)
        for p, t in enumerate(self.toks):
            self.logits[p] = m.transformer(int(t), p)
        kvd = c.dim // c.n_heads * c.n_kv_heads
        n = c.n_layers * c.seq_len * kvd
        self.k = m.state("key_cache", n).reshape(c.n_layers, c.seq_len, kvd)
        self.v = m.state("value_cache", n).reshape(c.n_layers, c.seq_len, kvd)
        m.close()


@pytest.fixture(scope="module")
def streams(ck, orc):
    with ThreadPoolExecutor(len(NAMES)) as ex:  # the oracle's calls release the GIL
        return dict(zip(NAMES, ex.map(lambda n: Stream(ck, orc, n), NAMES)))


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


def feed_history(s, w, toks, pos0, by_verify):
    """positions 0 .. pos0 - 1 of the stream: one l2z_prefill, or l2z_verify calls of up to 16 rows"""
    if pos0 == 0:
        return
    if not by_verify:
        s.prefill(toks[:pos0], 0, w)
        return
    p = 0
    while p < pos0:
        n = min(16, pos0 - p)
        s.verify(toks[p:p + n], p, w)
        p += n


def case_positions(seq_len, T):
    want = [0, 1, 17, SEG - 1, SEG, 5 * SEG + 220, min(300, seq_len - T), seq_len - T]
    out = []
    for p in want:
        if 0 <= p <= seq_len - T and p not in out:
            out.append(p)
    return out


# ---- 1. parity with the oracle's stepped pass, every row -------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_verify_parity_every_row(gpu, streams, name):
    st = streams[name]
    c = st.cfg
    w = gpu.Weights(c, st.blob, st.shared)
    case = 0
    worst = 0.0
    for T in TS:
        for pos0 in case_positions(c.seq_len, T):
            s = gpu.RunState(c)
            feed_history(s, w, st.toks, pos0, by_verify=(case % 2 == 1))
            case += 1
            k0, v0 = caches(s, c)
            rows = st.toks[pos0:pos0 + T]
            nxt, a = s.verify(rows, pos0, w)
            z = [s.verify_logits(i) for i in range(T)]
            for i in range(T):
                err = float(np.abs(z[i] - st.logits[pos0 + i]).max())
                worst = max(worst, err)
                np.testing.assert_allclose(z[i], st.logits[pos0 + i], rtol=LOGIT_RTOL, atol=LOGIT_ATOL,
                                           err_msg=f"{name} pos0 {pos0} T {T} row {i}")
                assert int(nxt[i]) == np_argmax(z[i])
            assert a == np_accept(rows, nxt)
            assert np.array_equal(bits(s.logits()), bits(z[a])), (name, pos0, T)
            assert s.argmax() == int(nxt[a])
            k1, v1 = caches(s, c)
            sl = slice(pos0, pos0 + T)
            np.testing.assert_allclose(k1[:, sl], st.k[:, sl], rtol=KV_TOL, atol=KV_TOL)
            np.testing.assert_allclose(v1[:, sl], st.v[:, sl], rtol=KV_TOL, atol=KV_TOL)
            keep = np.ones(c.seq_len, bool)
            keep[sl] = False
            assert np.array_equal(bits(k1[:, keep]), bits(k0[:, keep])), (name, pos0, T)
            assert np.array_equal(bits(v1[:, keep]), bits(v0[:, keep])), (name, pos0, T)
            s.close()
    print(f"verify parity {name}: {case} cases, max |logit diff| {worst:.3e}")
    w.close()


# ---- 2. the verdict is exact ---------------------------------------------------------------------------------------------

def greedy_by_single_rows(s, w, first_token, pos0, n):
    """n one-row verify calls from (first_token, pos0): the tokens fed, [n + 1] (the last one is not fed), and every
    position's logits row"""
    fed, rows = [int(first_token)], []
    for i in range(n):
        nxt, a = s.verify([fed[-1]], pos0 + i, w)
        assert a == 0
        rows.append(s.verify_logits(0))
        fed.append(int(nxt[0]))
    return fed, rows


def test_verdict_for_every_accept_length(gpu, ck):
    cfg = ck.STORIES15M
    w = gpu.Weights(cfg, None, True, seed=3)
    rng = np.random.default_rng(8)
    prompt = rng.integers(2, cfg.vocab_size, size=9).astype(np.int32)
    s = gpu.RunState(cfg)
    s.prefill(prompt[:8], 0, w)
    g, _ = greedy_by_single_rows(s, w, prompt[8], 8, 16)   # g[0] = prompt[8], g[1 ..] = the model's continuation
    for want in range(16):
        toks = np.array(g[:16], np.int32)
        if want < 15:
            toks[want + 1] = (toks[want + 1] + 1 - 2) % (cfg.vocab_size - 2) + 2   # a wrong guess
            toks[want + 2:] = rng.integers(2, cfg.vocab_size, size=max(0, 16 - want - 2))
        nxt, a = s.verify(toks, 8, w)
        z = [s.verify_logits(i) for i in range(16)]
        for i in range(16):
            assert int(nxt[i]) == np_argmax(z[i]), (want, i)
        assert a == np_accept(toks, nxt) == want
        assert nxt[:a + 1].tolist() == g[1:a + 2]
        assert s.argmax() == int(nxt[a])
    s.close(); w.close()


def test_planted_tie_resolves_to_the_lower_id(gpu, ck):
    """Classifier rows 7 and 4000 are copies of one row, scaled up so that it wins wherever its logit is positive: z[7] and
    z[4000] are the same bits.  The verdict says 7; a guess of 4000 is rejected, a guess of 7 accepted."""
    cfg = ck.STORIES15M
    blob = ck.synth_blob(cfg, False, seed=23)
    wcls = ck.carve(cfg, blob, False)["wcls"]
    wcls[7] *= np.float32(8.0)
    wcls[4000] = wcls[7]
    w, s = gpu.Weights(cfg, blob, False), gpu.RunState(cfg)
    rng = np.random.default_rng(4)
    toks = rng.integers(2, cfg.vocab_size, size=200).astype(np.int32)
    seen = 0
    for p in range(199):   # row 0 reads the stream's token at p; the row behind it holds the guess
        nxt, a = s.verify([toks[p], 4000], p, w)
        assert int(nxt[0]) != 4000
        if int(nxt[0]) == 7:
            z = s.verify_logits(0)
            assert bits(z)[7] == bits(z)[4000] and np_argmax(z) == 7
            assert a == 0, "the guess equal to the higher id of the tie must be rejected"
            nxt, a = s.verify([toks[p], 7], p, w)
            assert int(nxt[0]) == 7 and a == 1
            seen += 1
    # (the scaled row's logit is positive at about half of the positions and then beats the best of 32000 others often)
    assert seen >= 5, "the tied rows never held the maximum: the case shows nothing"
    s.close(); w.close()


# ---- 3. draft invariance, bit for bit --------------------------------------------------------------------------------------

def cut(pattern, n):
    """the pattern repeated and clipped to n positions"""
    out, i = [], 0
    while sum(out) < n:
        out.append(min(pattern[i % len(pattern)], n - sum(out)))
        i += 1
    return out


def invariance_runs(gpu, cfg, w, prefix, first_token, p0, n):
    """the n positions p0 .. of the model's own greedy continuation, processed four ways on fresh runstates; every
    position's logits row and every cache row 0 .. p0 + n - 1 must be the same bits"""
    def fresh():
        s = gpu.RunState(cfg)
        if p0:
            s.prefill(prefix, 0, w)
        return s

    s = fresh()
    g, rows_a = greedy_by_single_rows(s, w, first_token, p0, n)
    end = p0 + n
    ka, va = [x[:, :end].copy() for x in caches(s, cfg)]
    s.close()
    ref = [bits(r) for r in rows_a]
    g = np.array(g, np.int32)

    def same(s, rows, what):
        for i, r in enumerate(rows):
            assert np.array_equal(bits(r), ref[i]), (what, "logits of position", p0 + i)
        k, v = caches(s, cfg)
        assert np.array_equal(bits(k[:, :end]), bits(ka)), (what, "key cache")
        assert np.array_equal(bits(v[:, :end]), bits(va)), (what, "value cache")
        s.close()

    for pattern in ([16, 16, 16], [3, 7, 1, 13, 16, 8]):   # all guesses right
        s, rows, p = fresh(), [], 0
        for m in cut(pattern, n):
            nxt, a = s.verify(g[p:p + m], p0 + p, w)
            assert a == m - 1 and nxt.tolist() == g[p + 1:p + m + 1].tolist(), (pattern, p)
            rows += [s.verify_logits(i) for i in range(m)]
            p += m
        same(s, rows, pattern)
    # wrong guesses at planted places: calls end early, the next call starts behind the accepted tokens and overwrites the
    # rejected rows
    s, rows, p, call = fresh(), [], 0, 0
    rng = np.random.default_rng(12)
    while p < n:
        m = min((16, 9, 16, 5)[call % 4], n - p)
        t = g[p:p + m].copy()
        j = 1 + (call * 5) % 16   # the first wrong guess of this call (none if beyond its rows)
        if j < m:
            t[j] = (t[j] - 2 + 1 + int(rng.integers(0, 5))) % (cfg.vocab_size - 2) + 2
            t[j + 1:] = rng.integers(2, cfg.vocab_size, size=m - j - 1)
        nxt, a = s.verify(t, p0 + p, w)
        assert a == min(j, m) - 1, (call, a, j, m)
        rows += [s.verify_logits(i) for i in range(a + 1)]
        p += a + 1
        call += 1
    same(s, rows, "planted wrong guesses")


@pytest.mark.parametrize("name", NAMES)
def test_draft_invariance_bitwise(gpu, ck, name):
    cfg, shared, blob = model(ck, name)
    w = gpu.Weights(cfg, blob, shared)
    invariance_runs(gpu, cfg, w, None, 1, 0, min(48, cfg.seq_len))
    w.close()


def test_draft_invariance_across_two_segment_boundaries(gpu, ck):
    cfg, shared, blob = model(ck, "long_gqa")
    w = gpu.Weights(cfg, blob, shared)
    rng = np.random.default_rng(31)
    prefix = rng.integers(2, cfg.vocab_size, size=SEG - 6).astype(np.int32)
    invariance_runs(gpu, cfg, w, prefix, int(rng.integers(2, cfg.vocab_size)), SEG - 6, SEG + 16)   # 58 .. 137
    w.close()


# ---- 4. the loop ---------------------------------------------------------------------------------------------------------

def golden_models(ck):
    meta = json.load(open(os.path.join(GOLD, "toy_models.json")))
    for ent in meta["models"]:
        c, shared, blob = ck.read_checkpoint(os.path.join(GOLD, ent["checkpoint"]))
        yield ent, c, shared, np.ascontiguousarray(blob, np.float32)


def check_stats(toks, stats, n_prompt):
    assert stats["accepted"] <= stats["offered"]
    assert stats["emitted"] == len(toks) - n_prompt - 1          # the first generated token is l2z_argmax's
    assert stats["emitted"] <= stats["accepted"] + stats["calls"]  # = sum (a + 1), cut at a BOS or the step budget


@pytest.mark.parametrize("k", [0, 1, 4, 15])
def test_speculate_greedy_emits_the_golden_ids(gpu, ck, k):
    for ent, c, shared, blob in golden_models(ck):
        exp = np.load(os.path.join(GOLD, ent["expected"]))["tokens"]
        w, s = gpu.Weights(c, blob, shared), gpu.RunState(c)
        toks, stats = gpu.speculate_greedy(s, w, ent["prompt"], len(exp), k)
        assert toks.tolist() == exp.tolist(), (ent["checkpoint"], k)
        check_stats(toks, stats, len(ent["prompt"]))
        s.close(); w.close()


def test_speculate_greedy_does_not_depend_on_the_drafter(gpu, ck):
    cfg = ck.STORIES15M
    w = gpu.Weights(cfg, None, True, seed=15)
    prompt = [9, 400, 77, 2001, 15]
    steps = 200

    def run(k, drafter=None):
        s = gpu.RunState(cfg)
        toks, stats = gpu.speculate_greedy(s, w, prompt, steps, k, drafter)
        lg = bits(s.logits()).copy()
        s.close()
        check_stats(toks, stats, len(prompt))
        return toks, stats, lg

    base, st0, lg0 = run(0)
    assert st0["offered"] == 0 and st0["calls"] == st0["emitted"]
    full = np.concatenate([[1], base]).astype(np.int32)   # history as the drafter sees it
    rng = np.random.default_rng(6)
    count = [0]

    def replay(hist, k):
        return full[len(hist):len(hist) + k]

    def noise(hist, k):
        return rng.integers(2, cfg.vocab_size, size=k)

    def right_then_wrong(hist, k):
        j = count[0] % 15
        count[0] += 1
        g = full[len(hist):len(hist) + k].copy()
        if j < len(g):
            g[j:] = (g[j:] - 2 + 1) % (cfg.vocab_size - 2) + 2
        return g

    for what, k, d in (("lookup", 4, None), ("replay", 15, replay), ("noise", 15, noise), ("right then wrong", 15, right_then_wrong)):
        toks, stats, lg = run(k, d)
        assert toks.tolist() == base.tolist(), what
        if 1 not in base.tolist():   # (a BOS ends the run wherever it stands in a call; the step budget ends it at a call's end)
            assert np.array_equal(lg, lg0), what
        if what == "replay" and 1 not in base.tolist():
            assert stats["accepted"] == stats["offered"] and stats["calls"] <= (steps - len(prompt) - 1 + 15) // 16 + 1
        print(f"speculate {what} k={k}: {stats}")
    w.close()


def test_speculate_greedy_stops_after_a_bos_inside_an_accepted_run(gpu, ck):
    """The classifier's BOS row is a scaled copy of another row, so the model says BOS at many positions.  The raw API does
    not stop there: one-row verify calls give the continuation through it, a drafter that replays that continuation is always
    right, and the loop must still end with the BOS."""
    cfg = ck.STORIES15M
    blob = ck.synth_blob(cfg, False, seed=29)
    wcls = ck.carve(cfg, blob, False)["wcls"]
    wcls[1] = wcls[9] * np.float32(8.0)
    w = gpu.Weights(cfg, blob, False)
    rng = np.random.default_rng(17)
    done = 0
    for trial in range(12):
        prompt = [int(t) for t in rng.integers(2, cfg.vocab_size, size=4)]
        s = gpu.RunState(cfg)
        hist = np.array([1] + prompt, np.int32)
        s.prefill(hist, 0, w)
        g, _ = greedy_by_single_rows(s, w, s.argmax(), len(hist), 40)
        s.close()
        full = np.concatenate([hist, g]).astype(np.int32)
        where = [i for i in range(len(hist), len(full)) if full[i] == 1]
        if not where or where[0] < len(hist) + 3 or where[0] > len(full) - 4:
            continue
        m = where[0]
        s = gpu.RunState(cfg)
        toks, stats = gpu.speculate_greedy(s, w, prompt, 0, 15, lambda h, k: full[len(h):len(h) + k])
        s.close()
        assert toks.tolist() == full[1:m + 1].tolist() and toks[-1] == 1
        assert stats["accepted"] == stats["offered"]
        done += stats["emitted"] < stats["accepted"] + stats["calls"]   # rows behind the BOS were accepted too, and dropped
    assert done >= 2, "no run had a BOS inside an accepted run: the case shows nothing"
    w.close()


def test_speculate_greedy_stops_at_seq_len_with_a_shorter_last_call(gpu, ck):
    cfg = ck.Config(288, 768, 6, 6, 6, 32000, 64)
    for seed in range(15, 20):   # (a synthetic model that never says BOS inside its context: the first seed, most likely)
        w = gpu.Weights(cfg, None, True, seed=seed)
        s = gpu.RunState(cfg)
        base, _ = gpu.speculate_greedy(s, w, [5, 6], 0, 0)
        s.close()
        if 1 not in base.tolist():
            break
        w.close()
    assert 1 not in base.tolist() and len(base) == cfg.seq_len
    full = np.concatenate([[1], base]).astype(np.int32)
    asked = []

    def replay(hist, k):
        asked.append((len(hist), k))
        return full[len(hist):len(hist) + k]

    s = gpu.RunState(cfg)
    toks, stats = gpu.speculate_greedy(s, w, [5, 6], 0, 15, replay)
    assert toks.tolist() == base.tolist()
    for n_hist, k in asked:   # the call's rows are positions n_hist - 1 .. n_hist - 1 + k
        assert n_hist - 1 + k <= cfg.seq_len - 1
    assert 0 < asked[-1][1] < 15 and asked[-1][0] - 1 + asked[-1][1] == cfg.seq_len - 1
    s.close(); w.close()


def test_cli_spec_prints_what_plain_greedy_prints(gpu):
    exe = os.path.join(HOST, "llama2")
    for ckpt, prompt in (("toy_gqa_unshared.bin", None), ("toy_mha_shared.bin", "a b")):
        outs = []
        for extra in ([], ["--spec", "4"], ["--spec", "0"], ["--spec", "15"]):
            args = [exe, os.path.join(GOLD, ckpt), "-t", "0", "-n", "24", "-z", TOK, "-v", "--tokens", *extra]
            if prompt:
                args += ["-i", prompt]
            r = subprocess.run(args, capture_output=True, timeout=180)
            assert r.returncode == 0, r.stderr.decode(errors="replace")
            err = r.stderr.decode(errors="replace")
            outs.append(([l for l in err.splitlines() if l.startswith("tokens:")][0], r.stdout))
            assert ("spec:" in err) == bool(extra)
        for o in outs[1:]:
            assert o == outs[0], ckpt


# ---- 5. it composes ------------------------------------------------------------------------------------------------------

def test_verify_composes_with_the_other_entry_points(gpu, streams):
    """after a verify call that rejected guesses, each of the other entry points continues at pos0 + a + 1 and meets the oracle"""
    st = streams["stories15M"]
    c = st.cfg
    w = gpu.Weights(c, st.blob, st.shared)
    pos0 = 40

    def after_verify():
        s = gpu.RunState(c)
        s.prefill(st.toks[:pos0], 0, w)
        rows = st.toks[pos0:pos0 + 8].copy()
        nxt, a = s.verify(rows, pos0, w)
        assert a < 7   # random guesses: rejected (rows a + 1 .. 7 are stale now)
        # continue the STREAM: its token at pos0 + a + 1 (the stream is the sequence here, the model's own pick is not)
        return s, pos0 + a + 1, int(nxt[a])

    def close(z, p):
        np.testing.assert_allclose(z, st.logits[p], rtol=LOGIT_RTOL, atol=LOGIT_ATOL)

    s, p, top = after_verify()
    assert gpu.sample_batch([s], 0.0, 0.9, 0.5).tolist() == [top] and s.argmax() == top
    s.transformer(int(st.toks[p]), p, w)
    close(s.logits(), p)
    s.close()

    s, p, _ = after_verify()
    comp = gpu.RunState(c)
    gpu.transformer_batch([comp, s], [5, int(st.toks[p])], [0, p], w)
    close(s.logits(), p)
    s.close(); comp.close()

    s, p, _ = after_verify()
    s.prefill(st.toks[p:p + 6], p, w)
    close(s.logits(), p + 5)
    s.close()

    s, p, _ = after_verify()
    dst = gpu.RunState(c)
    gpu.runstate_fork(dst, s, p)
    assert np.array_equal(bits(dst.logits()), bits(s.logits()))
    dst.transformer(int(st.toks[p]), p, w)
    close(dst.logits(), p)
    nxt, _ = dst.verify(st.toks[p + 1:p + 4], p + 1, w)
    close(dst.verify_logits(2), p + 3)
    s.close(); dst.close()
    w.close()


# ---- 6. refusals change nothing --------------------------------------------------------------------------------------------

def test_verify_contract_violations_change_nothing(gpu, ck):
    import ctypes as C
    c = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    c2 = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=16)
    odd = ck.Config(dim=64, hidden_dim=174, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=32)
    w = gpu.Weights(c, None, False, seed=4)
    w_odd = gpu.Weights(odd, None, False, seed=4)
    s = gpu.RunState(c)
    s_odd = gpu.RunState(odd)
    s.prefill(np.array([3, 4, 5], np.int32), 0, w)
    s.verify([6, 7], 3, w)   # (the scratch exists: a refusal must not touch it either)
    comm = gpu.Comm(0, 2, None, 0, emulated=True)
    shard = gpu.RunState(c, comm)

    def snap():
        return (np.concatenate([x.ravel() for x in caches(s, c)]).view(np.uint32), bits(s.logits()).copy(),
                bits(s.verify_logits(1)).copy())
    before = snap()
    L = gpu.lib()
    i32p = C.POINTER(C.c_int32)
    cfg_c = s.cfg
    cfg_2 = gpu.L2ZConfig(*[int(v) for v in c2.as_i32()])
    out = (C.c_int32 * 17)()
    acc = C.c_int(0)

    def call(tokens, n, pos0, cfg=cfg_c, state=s, weights=w, o=out, a=C.byref(acc)):
        t = np.array(tokens if tokens is not None else [0], np.int32)
        return L.l2z_verify(t.ctypes.data_as(i32p) if tokens is not None else None, n, pos0, C.byref(cfg),
                            state.h if state is not None else None, weights.h if weights is not None else None, o, a)

    cases = [
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
    ]
    for kw, code, what in cases:
        assert call(**kw) == code, what
    with pytest.raises(gpu.L2ZError) as e:
        s.verify_logits(2)   # the last call had two rows
    assert e.value.code == gpu.ERR_STATE
    after = snap()
    for b0, b1 in zip(before, after):
        assert np.array_equal(b0, b1)
    assert call([1, 2], 2, 30) == gpu.OK   # the last two positions are a valid call
    for x in (s, s_odd, shard):
        x.close()
    comm.close()
    w.close(); w_odd.close()
