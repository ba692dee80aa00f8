"""l2z_sample_run on the GPU: the sampled generation loop on the device (RunState.sample_run, binding.generate_sample).

The reference is the STEPPED ROUTE: per position l2z_transformer(token, pos), then prompt[pos] or the token
sample_batch([s], t, p, coin) draws from the logits (l2z_argmax for a greedy stretch); where the loop prefills -- the first
call after greedy_begin covers a prompt of L2Z_PREFILL_MIN_PROMPT tokens or more that holds no BOS -- the prompt goes through
RunState.prefill.  Every comparison is exact (np.array_equal on ids, uint32 compares on floats): there is no tolerance.

Models, the smallest that reach each branch: a wide-vocabulary toy (vocab 8259: above the prefix walk's 8192-value staging
and no multiple of 64, so the walk takes two stagings and the tails are live; seq_len 320, so a run crosses the attention
variants' switch-overs), a small GQA toy (vocab 259, seq_len 64), and the stories15M shape (the fused small-model launch sits
in the step graph)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFILL_MIN_PROMPT = 4   # include/llama2_hip.h L2Z_PREFILL_MIN_PROMPT
NAMES = ("wide", "small", "stories15M")
TPS = ((1.0, 0.9), (1.0, 1.0), (1.0, 0.0), (0.05, 0.9), (0.7, 0.5))
PROMPTS = ((), (5, 9, 7), (5, 9, 7, 11, 13, 17, 19, 23, 29))


def config(ck, name):
    return {"wide": ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=4, vocab_size=8259, seq_len=320),
            "small": ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=259, seq_len=64),
            "stories15M": ck.STORIES15M}[name]


@pytest.fixture(scope="module")
def models(gpu, ck):
    """name -> (config, weights, runstate of the loop, runstate of the stepped route); made on first use, shared"""
    made = {}

    def get(name):
        if name not in made:
            cfg = config(ck, name)
            made[name] = (cfg, gpu.Weights(cfg, None, True, seed=77), gpu.RunState(cfg), gpu.RunState(cfg))
        return made[name]
    yield get
    for cfg, w, s, r in made.values():
        s.close(); r.close(); w.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def caches(s, c, rows):
    """rows 0 .. rows - 1 of the runstate's caches in the reference's order [layer, seq_len, kv_dim]"""
    kvd = c.dim // c.n_heads * c.n_kv_heads
    n = c.n_layers * c.seq_len * kvd
    return [s.read(name, 0, n).reshape(c.n_layers, c.seq_len, kvd)[:, :rows].copy() for name in ("key_cache", "value_cache")]


def step_coins(gpu, seed, prompt, steps):
    """one coin per step: 0 at the prompt's steps, then coin_stream(seed) in generation order (generate_sample's mapping)"""
    out = np.zeros(steps, np.float32)
    n_gen = max(0, steps - len(prompt))
    out[len(prompt):] = gpu.coin_stream(seed, n_gen)
    return out


class Stepped:
    """The stepped route on runstate r, from BOS + prompt: run(n, t, p, coins) takes the next n steps -- coins[i] for step i of
    the call -- and returns their ids; t == 0 is a greedy stretch (l2z_argmax).  pick: another rule for a generated token,
    (runstate) -> id."""

    def __init__(self, gpu, r, w, prompt, seq_len):
        self.gpu, self.r, self.w, self.prompt, self.seq_len = gpu, r, w, [int(t) for t in prompt], seq_len
        self.pos, self.token, self.done = 0, 1, False

    def run(self, n, t, p, coins=None, pick=None):
        out = []
        n = min(n, self.seq_len - self.pos)
        if self.done or n <= 0:
            return np.array(out, np.int32)
        np_ = len(self.prompt)
        if self.pos == 0 and np_ >= PREFILL_MIN_PROMPT and n >= np_ and 1 not in self.prompt:
            self.r.prefill(np.array([1] + self.prompt[:-1], np.int32), 0, self.w)
            out += self.prompt
            self.pos, self.token = np_, self.prompt[-1]
        first = self.pos - len(out)
        while len(out) < n and not self.done:
            self.r.transformer(self.token, self.pos, self.w)
            if self.pos < np_:
                nxt = self.prompt[self.pos]
            elif pick is not None:
                nxt = pick(self.r)
            elif t == 0:
                nxt = self.r.argmax()
            else:
                nxt = int(self.gpu.sample_batch([self.r], t, p, coins[self.pos - first])[0])
            out.append(int(nxt))
            self.pos += 1
            self.token = int(nxt)
            self.done = nxt == 1
        return np.array(out, np.int32)


# ---- 1. the loop equals the stepped route ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_loop_equals_the_stepped_route(gpu, models, name):
    """40 steps from every prompt length (none, 3 tokens: stepped prompt, 9 tokens: prefilled prompt) with every (t, p):
    the ids, and the logits the last step left, bit for bit, for EVERY combination.  A run that a drawn BOS ends leaves the
    logits of its chunk's last step, not of the BOS's, so a combination takes the first of its coin seeds (base, base + 1, ...)
    whose stepped run goes all 40 steps; the seeds passed over on the way are runs a drawn BOS ends, and their ids are
    compared too."""
    cfg, w, s, r = models(name)
    steps = 40
    for pi, prompt in enumerate(PROMPTS):
        for ti, (t, p) in enumerate(TPS):
            base = 100 + 100 * pi + 10 * ti
            for seed in range(base, base + 8):
                ids = gpu.generate_sample(s, w, prompt, steps, t, p, gpu.coin_stream(seed, steps))
                ref = Stepped(gpu, r, w, prompt, cfg.seq_len).run(steps, t, p, step_coins(gpu, seed, prompt, steps))
                assert np.array_equal(ids, ref), (name, prompt, t, p, seed, ids, ref)
                assert list(ids[:len(prompt)]) == list(prompt)
                if ids[-1] != 1:
                    break
            assert len(ids) == steps and ids[-1] != 1, (name, prompt, t, p, "eight coin seeds in a row drew a BOS")
            assert np.array_equal(bits(s.logits()), bits(r.logits())), (name, prompt, t, p, seed)


# ---- 2. split invariance --------------------------------------------------------------------------------------------------

def test_split_invariance(gpu, models):
    """150 steps in one call = the same steps cut into calls of 1, 7, 64 and 78 steps with the same per-position coins: ids,
    the last logits and the KV rows below the last position."""
    cfg, w, s, r = models("wide")
    prompt, steps, t, p = (5, 9, 7), 150, 1.0, 0.9
    coins = step_coins(gpu, 7, prompt, steps)
    s.greedy_begin(prompt)
    whole = s.sample_run(w, steps, t, p, coins)
    assert len(whole) == steps and whole[-1] != 1, "a drawn BOS ended the run: take another coin seed"
    z, kv = bits(s.logits()).copy(), caches(s, cfg, steps)
    r.greedy_begin(prompt)
    parts, at = [], 0
    for n in (1, 7, 64, 78):
        parts.append(r.sample_run(w, n, t, p, coins[at: at + n]))
        assert len(parts[-1]) == n
        at += n
    assert at == steps
    assert np.array_equal(np.concatenate(parts), whole)
    assert np.array_equal(bits(r.logits()), z)
    for a, b in zip(caches(r, cfg, steps), kv):
        assert np.array_equal(bits(a), bits(b))


# ---- 3. across the attention variants -------------------------------------------------------------------------------------

def test_a_run_across_the_attention_variants(gpu, models):
    """310 steps on the seq_len-320 model: the run crosses the switch-overs of the attention form (short, one block per
    head, split), so the sampled step's graph of a later variant is captured in the middle of the sequence."""
    cfg, w, s, r = models("wide")
    steps, t, p = 310, 1.0, 0.9
    coins = gpu.coin_stream(31, steps)
    ids = gpu.generate_sample(s, w, (), steps, t, p, coins)
    ref = Stepped(gpu, r, w, (), cfg.seq_len).run(steps, t, p, coins)
    assert np.array_equal(ids, ref)
    assert len(ids) == steps and ids[-1] != 1, "a drawn BOS ended the run: take another coin seed"
    assert np.array_equal(bits(s.logits()), bits(r.logits()))


# ---- 4. temperature 0 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_temperature_0_is_the_greedy_loop(gpu, models, name):
    cfg, w, s, r = models(name)
    for prompt in PROMPTS:
        r.greedy_begin(prompt)
        ref = r.greedy_run(w, 40)
        s.greedy_begin(prompt)
        ids = s.sample_run(w, 40, 0.0, 0.9, None)
        assert np.array_equal(ids, ref), (name, prompt)


# ---- 5. greedy and sampled calls alternate --------------------------------------------------------------------------------

def test_greedy_and_sampled_calls_alternate(gpu, models):
    cfg, w, s, r = models("small")
    prompt, t, p = (5, 9, 7), 0.7, 0.5
    coins = gpu.coin_stream(5, 10)
    s.greedy_begin(prompt)
    ids = np.concatenate([s.greedy_run(w, 10), s.sample_run(w, 10, t, p, coins), s.greedy_run(w, 10)])
    st = Stepped(gpu, r, w, prompt, cfg.seq_len)
    ref = np.concatenate([st.run(10, 0.0, 1.0), st.run(10, t, p, coins), st.run(10, 0.0, 1.0)])
    assert np.array_equal(ids, ref)
    assert len(ids) == 30 or ids[-1] == 1
    if ids[-1] != 1:
        assert np.array_equal(bits(s.logits()), bits(r.logits()))


# ---- 6. the argmax fallback -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("wide", "small"))
def test_a_tiny_top_p_takes_the_most_probable_token(gpu, models, name):
    """top_p = 1e-6 is below 1 / vocab: the first candidate alone exceeds it (or no token passes the cutoff), so the token
    is the most probable one (lowest id among equals) whatever the coin."""
    cfg, w, s, r = models(name)
    t, p, steps = 0.05, 1e-6, 24
    assert p < 1.0 / cfg.vocab_size
    a = gpu.generate_sample(s, w, (), steps, t, p, gpu.coin_stream(1, steps))
    b = gpu.generate_sample(s, w, (), steps, t, p, gpu.coin_stream(2, steps))
    assert np.array_equal(a, b)

    def most_probable(rs):
        pr = rs.probs(t)
        return int(np.flatnonzero(pr == pr.max())[0])
    ref = Stepped(gpu, r, w, (), cfg.seq_len).run(steps, t, p, pick=most_probable)
    assert np.array_equal(a, ref)


# ---- 7. coins of prompt steps ---------------------------------------------------------------------------------------------

def test_coins_of_prompt_steps_are_ignored(gpu, models):
    cfg, w, s, r = models("small")
    t, p, steps = 1.0, 0.9, 24
    for prompt in PROMPTS[1:]:
        coins = step_coins(gpu, 9, prompt, steps)
        other = coins.copy()
        other[:len(prompt)] = np.linspace(0.05, 0.95, len(prompt), dtype=np.float32)
        s.greedy_begin(prompt)
        a = s.sample_run(w, steps, t, p, coins)
        s.greedy_begin(prompt)
        b = s.sample_run(w, steps, t, p, other)
        assert np.array_equal(a, b), prompt


# ---- 8. BOS ---------------------------------------------------------------------------------------------------------------

def test_a_bos_ends_the_run(gpu, models):
    cfg, w, s, r = models("small")
    coins = gpu.coin_stream(3, 20)
    s.greedy_begin([5, 9, 1, 7])   # holds a BOS: the prompt stays stepped
    ids = s.sample_run(w, 20, 1.0, 0.9, coins)
    assert list(ids) == [5, 9, 1]
    assert len(s.sample_run(w, 20, 1.0, 0.9, coins)) == 0
    assert len(s.greedy_run(w, 20)) == 0
    ref = Stepped(gpu, r, w, (5, 9), cfg.seq_len).run(20, 1.0, 0.9, step_coins(gpu, 3, (5, 9), 20))
    s.greedy_begin([5, 9])
    assert np.array_equal(s.sample_run(w, 20, 1.0, 0.9, step_coins(gpu, 3, (5, 9), 20)), ref)


# ---- 9. the end of the context --------------------------------------------------------------------------------------------

def test_the_end_of_the_context(gpu, models):
    cfg, w, s, r = models("small")
    t, p = 0.05, 0.9
    coins = gpu.coin_stream(4, 200)
    ref = Stepped(gpu, r, w, (), cfg.seq_len).run(cfg.seq_len, t, p, coins)
    assert len(ref) == cfg.seq_len and ref[-1] != 1, "a drawn BOS ended the run: take another coin seed"
    s.greedy_begin(())
    a = s.sample_run(w, 50, t, p, coins[:50])
    b = s.sample_run(w, 100, t, p, coins[50:150])   # 14 positions are left
    assert len(a) == 50 and len(b) == cfg.seq_len - 50
    assert np.array_equal(np.concatenate([a, b]), ref)
    assert len(s.sample_run(w, 5, t, p, coins[:5])) == 0
    assert len(gpu.generate_sample(s, w, (), 200, t, p, coins)) == cfg.seq_len


# ---- 10. without graphs ---------------------------------------------------------------------------------------------------

_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package()
B, ck = pkg.binding, pkg.checkpoint
cfg = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=259, seq_len=64)
w = B.Weights(cfg, None, True, seed=77)
s = B.RunState(cfg)
out = []
for prompt in ((), (5, 9, 7), (5, 9, 7, 11, 13, 17, 19, 23, 29)):
    out.append([int(t) for t in B.generate_sample(s, w, prompt, 40, 0.7, 0.5, B.coin_stream(11, 40))])
print(json.dumps(out))
"""


def test_without_graphs_the_ids_are_the_same(gpu, models):
    cfg, w, s, r = models("small")
    env = dict(os.environ, L2Z_NO_GRAPH="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    eager = json.loads(out.strip().splitlines()[-1])
    for prompt, ids in zip(PROMPTS, eager):
        assert [int(t) for t in gpu.generate_sample(s, w, prompt, 40, 0.7, 0.5, gpu.coin_stream(11, 40))] == ids, prompt


# ---- 11. refusals change nothing ------------------------------------------------------------------------------------------

def test_refusals_change_nothing(gpu, ck, models):
    cfg, w, s, twin = models("small")
    good = gpu.coin_stream(6, 8)
    for x in (s, twin):
        x.greedy_begin((5, 9, 7))
        x.sample_run(w, 8, 1.0, 0.9, good)   # (the scratch and a graph exist: a refusal must not touch them either)
    comm = gpu.Comm(0, 2, None, 0, emulated=True)
    cfg2 = ck.Config(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=64)   # (splits over 2 ranks)
    w_shard = gpu.Weights(cfg2, None, True, seed=77, comm=comm)
    shard = gpu.RunState(cfg2, comm)
    L = gpu.lib()
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    out = (C.c_int32 * 8)()
    n = C.c_int(-7)
    nan = float("nan")

    def call(steps=8, t=1.0, p=0.9, coins=good, state=s, weights=w, o=out, on=C.byref(n)):
        cc = np.ascontiguousarray(coins, np.float32) if coins is not None else None
        return L.l2z_sample_run(C.byref(state.cfg) if state is not None else C.byref(s.cfg), state.h if state is not None else None,
                                weights.h if weights is not None else None, steps, C.c_float(t), C.c_float(p),
                                cc.ctypes.data_as(fp) if cc is not None else None, o, on)

    def last(v):
        c = good.copy()
        c[-1] = v
        return c
    cases = [(dict(t=nan), "temperature NaN"), (dict(t=float("inf")), "temperature inf"), (dict(t=-0.5), "temperature < 0"),
             (dict(p=1.5), "top_p 1.5"), (dict(p=-0.1), "top_p < 0"), (dict(p=nan), "top_p NaN"),
             (dict(coins=None), "NULL coins at t > 0"), (dict(coins=last(1.0)), "last coin 1.0"),
             (dict(coins=last(nan)), "last coin NaN"), (dict(coins=last(-0.25)), "last coin < 0"),
             (dict(steps=-1), "n_steps < 0"), (dict(state=None), "NULL runstate"), (dict(weights=None), "NULL weights"),
             (dict(o=None), "NULL out_tokens"), (dict(on=None), "NULL out_n"),
             (dict(state=shard, weights=w_shard), "a sharded runstate")]
    for kw, what in cases:
        assert call(**kw) == gpu.ERR_INVALID, what
    assert n.value == -7   # a refusal does not even write the count
    more = gpu.coin_stream(8, 8)
    assert np.array_equal(s.sample_run(w, 8, 0.7, 0.5, more), twin.sample_run(w, 8, 0.7, 0.5, more))
    assert np.array_equal(bits(s.logits()), bits(twin.logits()))
    shard.close(); w_shard.close(); comm.close()
