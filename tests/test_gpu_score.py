"""l2z_score on the GPU: every position's log-prob of its target and top-1 id from one batched pass.

The reference is the CPU oracle's stepped pass: its f32 logits z_i of every position, the expected log-prob computed from
them in float64.  THE BAR: |dlogprob_i| <= 2 * (LOGIT_ATOL + LOGIT_RTOL * max_v |z_i[v]|), the two constants of
tests/test_gpu_parity.py -- the project's bar on one logit, taken once for the target's logit and once for the
log-sum-exp (a 1-Lipschitz function of the logits in the max norm); the f32 summation of <= 32000 terms <= 1 adds < 1e-6
and is inside the factor.  Top-1 is compared wherever the oracle's margin (best - second logit) exceeds the same bar; at
most 2 % of a case's positions may fall under it.  State: KV rows and logits bit-identical to l2z_prefill's.  No figure
observed on the device sets any bound here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_gpu_parity import LOGIT_ATOL, LOGIT_RTOL, PREFILL_CONFIGS, SHARDED_PREFILL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "llama2.zig_amd", "host")
EXE = os.path.join(HOST, "llama2")
TOK = os.path.join(ROOT, "tests", "golden", "tokenizer.bin")

SMALL = dict(dim=288, hidden_dim=768, n_layers=2, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=320)
GQA = dict(next(c for c in SHARDED_PREFILL if c[0] == "gqa")[1])
STREAMS = dict(next(c for c in PREFILL_CONFIGS if c[0] == "streams-2048")[1])
SHAPES = {"small": SMALL, "gqa": GQA, "streams-2048": STREAMS}

# id -> (shape, shared weights, tokens, L2Z_PF_X3, forced slab columns (0: default), lengths of the calls)
CASES = {
    **{f"small-{t}": ("small", False, t, 1, 0, None) for t in (1, 5, 17, 40, 100, 300)},
    # 32000 columns in slabs of 8192: four slabs, the last one 7424 wide
    "small-300-slab8192": ("small", False, 300, 1, 8192, None),
    "small-100-slab4096": ("small", False, 100, 1, 4096, None),
    "gqa-530": ("gqa", False, 530, 1, 0, None),                 # two chunks
    "streams-2048-160": ("streams-2048", False, 160, 1, 0, None),   # layers on the bf16 cores
    "streams-2048-530": ("streams-2048", False, 530, 1, 0, None),
    "small-100-x3": ("small", False, 100, 2, 0, None),          # the classifier product on the bf16 cores: stream form
    "small-300-x3": ("small", False, 300, 2, 0, None),          # ... and the tile forms
    "small-300-x3-slab8192": ("small", False, 300, 2, 8192, None),
    "small-300-shared": ("small", True, 300, 1, 0, None),       # the classifier is the embedding
    "small-100-two-calls": ("small", False, 100, 1, 0, (9, 91)),
}
TOP1_CASES = ("small-300", "gqa-530", "streams-2048-160", "streams-2048-530", "small-300-x3", "small-300-shared",
              "small-300-slab8192")


def case_tokens(cfg, T):
    return np.array([1] + np.random.default_rng(4).integers(2, cfg.vocab_size, T - 1).tolist(), np.int32)


def bar_of(zmax):
    return 2.0 * (LOGIT_ATOL + LOGIT_RTOL * zmax)


_ORACLE = {}


def oracle_rows(orc, ck, shape, shared, T):
    """Per position of the oracle's stepped pass: float64 log-prob of the next token (NaN for the last), argmax, margin
    (best - second logit), max |logit|."""
    key = (shape, shared, T)
    if key in _ORACLE:
        return _ORACLE[key]
    cfg = ck.Config(**SHAPES[shape])
    blob = ck.synth_blob(cfg, shared, seed=23)
    toks = case_tokens(cfg, T)
    m = orc.Model(cfg.as_i32(), blob, shared)
    lp, top, margin, zmax = np.full(T, np.nan), np.zeros(T, np.int64), np.zeros(T), np.zeros(T)
    for i in range(T):
        z = m.transformer(int(toks[i]), i).astype(np.float64)
        mx = z.max()
        lse = mx + np.log(np.exp(z - mx).sum())
        if i + 1 < T:
            lp[i] = z[toks[i + 1]] - lse
        top[i] = int(np.argmax(z))
        two = np.partition(z, -2)[-2:]
        margin[i], zmax[i] = two[1] - two[0], np.abs(z).max()
    m.close()
    _ORACLE[key] = (lp, top, margin, zmax)
    return _ORACLE[key]


_SCORED = {}


def scored(gpu, ck, options, case):
    """(logprob, top1) of the case from the GPU, the calls' outputs concatenated."""
    shape, shared, T, x3, slab, calls = CASES[case]
    options(L2Z_PF_X3=x3)
    if case in _SCORED:
        return _SCORED[case]
    cfg = ck.Config(**SHAPES[shape])
    w = gpu.Weights(cfg, ck.synth_blob(cfg, shared, seed=23), shared)
    s = gpu.RunState(cfg)
    if slab:
        s.score_slab_set(slab)
    toks = case_tokens(cfg, T)
    targets = np.append(toks[1:], -1).astype(np.int32)
    lps, tops, pos0 = [], [], 0
    for n in calls or (T,):
        lp, top = s.score(toks[pos0:pos0 + n], pos0, w, targets=targets[pos0:pos0 + n])
        lps.append(lp); tops.append(top); pos0 += n
    s.close(); w.close()
    _SCORED[case] = (np.concatenate(lps), np.concatenate(tops))
    return _SCORED[case]


@pytest.mark.parametrize("case", list(CASES))
def test_logprob_parity_with_the_oracle(gpu, ck, orc, options, case):
    shape, shared, T, _, _, _ = CASES[case]
    lp, _ = scored(gpu, ck, options, case)
    ref, _, _, zmax = oracle_rows(orc, ck, shape, shared, T)
    assert lp[T - 1] == 0.0 and np.isfinite(lp).all()
    err = np.abs(lp[:T - 1].astype(np.float64) - ref[:T - 1])
    bar = bar_of(zmax[:T - 1])
    if T > 1:
        k = int(np.argmax(err / bar))
        print(f"score parity {case}: max |dlogprob| {err.max():.3e} (worst against its bar: {err[k]:.3e} of {bar[k]:.3e} "
              f"at position {k}), max |z| {zmax.max():.2f}, log-probs {ref[:T - 1].min():.2f} .. {ref[:T - 1].max():.2f}")
    assert np.all(err <= bar), (case, float(err.max()))


@pytest.mark.parametrize("case", TOP1_CASES)
def test_top1_equals_the_oracle_argmax_outside_near_ties(gpu, ck, orc, options, case):
    shape, shared, T, _, _, _ = CASES[case]
    _, top = scored(gpu, ck, options, case)
    _, ref, margin, zmax = oracle_rows(orc, ck, shape, shared, T)
    clear = margin > bar_of(zmax)
    print(f"score top-1 {case}: {int((~clear).sum())} of {T} positions under the bar, smallest margin {margin.min():.3e}")
    assert (~clear).sum() <= 0.02 * T, "vacuous: too many positions left out"
    assert np.array_equal(top[clear], ref[clear])
    assert ((top >= 0) & (top < SHAPES[shape]["vocab_size"])).all()


@pytest.mark.parametrize("slab", [0, 4096])
def test_tied_classifier_rows_resolve_to_the_lowest_index(gpu, ck, options, slab):
    """Classifier rows 7, 4000 and 20000 are copies of one row (scaled up so that it wins wherever its logit is positive):
    equal logits in two waves of one segment and in another segment (another slab when forced to 4096 columns).  Top-1 is
    7 there, never 4000 or 20000."""
    options(L2Z_PF_X3=1)
    cfg = ck.Config(**SMALL)
    blob = ck.synth_blob(cfg, False, seed=23)
    wcls = ck.carve(cfg, blob, False)["wcls"]
    wcls[7] *= np.float32(8.0)
    wcls[4000] = wcls[7]
    wcls[20000] = wcls[7]
    w, s = gpu.Weights(cfg, blob, False), gpu.RunState(cfg)
    if slab:
        s.score_slab_set(slab)
    toks = case_tokens(cfg, 300)
    _, top = s.score(toks, 0, w)
    s.close(); w.close()
    # (the scaled row's logit is 8 x a zero-mean value of the other logits' spread: it is positive at about half of the
    # positions and beats the best of 32000 others at roughly a third -- far more than 10 of 300)
    assert (top == 7).sum() >= 10, "the tied rows never held the maximum: the case shows nothing"
    assert not np.isin(top, (4000, 20000)).any()


def kv_and_logits(s, cfg):
    n = cfg.n_layers * cfg.seq_len * cfg.kv_dim
    return s.logits(), s.read("key_cache", 0, n), s.read("value_cache", 0, n)


@pytest.mark.parametrize("shape,T,calls", [("small", 300, (300,)), ("small", 100, (9, 91)), ("streams-2048", 160, (160,)),
                                           ("streams-2048", 530, (9, 521))],
                         ids=["small-300", "small-two-calls", "streams-2048-160", "streams-2048-two-calls"])
def test_state_is_prefills_bit_for_bit(gpu, ck, options, shape, T, calls):
    options(L2Z_PF_X3=1)
    cfg = ck.Config(**SHAPES[shape])
    w = gpu.Weights(cfg, None, False, seed=23)
    a, b = gpu.RunState(cfg), gpu.RunState(cfg)
    toks = case_tokens(cfg, T)
    pos0 = 0
    for n in calls:
        a.score(toks[pos0:pos0 + n], pos0, w)
        b.prefill(toks[pos0:pos0 + n], pos0, w)
        pos0 += n
        for x, y in zip(kv_and_logits(a, cfg), kv_and_logits(b, cfg)):
            assert np.array_equal(x, y)
    ids = []
    for s in (a, b):
        out, tok = [], s.argmax()
        for pos in range(T, T + 8):
            out.append(tok)
            s.transformer(tok, pos, w)
            tok = s.argmax()
        ids.append(out + [tok])
    assert ids[0] == ids[1]
    a.close(); b.close(); w.close()


def test_7b_score_agrees_with_the_stepped_gpu_path(gpu, ck):
    """The full 7B shape (seeded weights generated on the device): 300 tokens scored in one call; at six positions the
    stepped path's logits (l2z_transformer, read back) give the log-prob in float64 on the host; same bar.  The call
    leaves l2z_argmax where l2z_prefill leaves it."""
    cfg = ck.LLAMA2_7B
    w = gpu.Weights(cfg, None, False, seed=2024)
    s, st, sp = gpu.RunState(cfg), gpu.RunState(cfg), gpu.RunState(cfg)
    T = 300
    toks = case_tokens(cfg, T)
    lp, top = s.score(toks, 0, w)
    check = (0, 1, 63, 150, 257, 298)
    for i in range(max(check) + 1):
        st.transformer(int(toks[i]), i, w)
        if i not in check:
            continue
        z = st.logits().astype(np.float64)
        ref = z[toks[i + 1]] - (z.max() + np.log(np.exp(z - z.max()).sum()))
        bar = bar_of(np.abs(z).max())
        two = np.partition(z, -2)[-2:]
        print(f"7B score position {i}: logprob {lp[i]:.6f} vs stepped {ref:.6f} (|d| {abs(lp[i] - ref):.3e}, bar {bar:.3e}), "
              f"top-1 {top[i]} vs {int(np.argmax(z))}, margin {two[1] - two[0]:.3e}")
        assert abs(float(lp[i]) - ref) <= bar
        if two[1] - two[0] > bar:
            assert top[i] == int(np.argmax(z))
    sp.prefill(toks, 0, w)
    assert s.argmax() == sp.argmax()
    assert np.array_equal(s.logits(), sp.logits())
    for x in (s, st, sp):
        x.close()
    w.close()


TOY = dict(dim=64, hidden_dim=172, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512, seq_len=96)


def test_contract(gpu, ck, options):
    options(L2Z_PF_X3=1)
    L = gpu.lib()
    cfg = ck.Config(**TOY)
    w, s = gpu.Weights(cfg, None, False, seed=23), gpu.RunState(cfg)
    toks = case_tokens(cfg, 20)
    s.prefill(toks[:5], 0, w)
    before = kv_and_logits(s, cfg)
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    lp, top = np.zeros(32, np.float32), np.zeros(32, np.int32)

    def call(tokens, n, pos0, targets, out_lp, out_top, state=s, weights=w, c=None):
        p = lambda a, t: None if a is None else np.ascontiguousarray(a).ctypes.data_as(t)
        return L.l2z_score(p(tokens, i32p), n, pos0, p(targets, i32p), C.byref(c or state.cfg), state.h, weights.h,
                           p(out_lp, fp), p(out_top, i32p))

    t8, g8 = toks[5:13].copy(), toks[6:14].copy()
    assert call(None, 8, 5, g8, lp, top) == gpu.ERR_INVALID
    assert call(t8, 0, 5, g8, lp, top) == gpu.ERR_INVALID
    assert call(t8, 8, 5, None, None, None) == gpu.ERR_INVALID            # both outputs absent
    assert call(t8, 8, 5, g8, None, top) == gpu.ERR_INVALID               # targets without out_logprob
    assert call(t8, 8, 5, None, lp, top) == gpu.ERR_INVALID               # out_logprob without targets
    assert call(t8, 8, -1, g8, lp, top) == gpu.ERR_STATE
    assert call(t8, 8, cfg.seq_len - 7, g8, lp, top) == gpu.ERR_STATE
    bad = t8.copy(); bad[3] = cfg.vocab_size
    assert call(bad, 8, 5, g8, lp, top) == gpu.ERR_STATE
    bad = t8.copy(); bad[0] = -1
    assert call(bad, 8, 5, g8, lp, top) == gpu.ERR_STATE
    for v in (-2, cfg.vocab_size):
        bad = g8.copy(); bad[7] = v
        assert call(t8, 8, 5, bad, lp, top) == gpu.ERR_STATE
    # a sharded runstate (comm != NULL), with its own weights
    comm = gpu.Comm(0, 2, None, 0, emulated=True)
    ws, ss = gpu.Weights(cfg, None, False, seed=23, comm=comm), gpu.RunState(cfg, comm=comm)
    assert call(t8, 8, 0, g8, lp, top, state=ss, weights=ws) == gpu.ERR_INVALID
    ss.close(); ws.close(); comm.close()
    # dims l2z_prefill refuses
    odd = ck.Config(**dict(TOY, hidden_dim=174))
    wo, so = gpu.Weights(odd, None, False, seed=23), gpu.RunState(odd)
    assert call(t8, 8, 0, g8, lp, top, state=so, weights=wo) == gpu.ERR_INVALID
    with pytest.raises(gpu.L2ZError):
        so.prefill(t8, 0, wo)
    so.close(); wo.close()
    for x, y in zip(before, kv_and_logits(s, cfg)):
        assert np.array_equal(x, y)

    # no target: exactly 0.0; the other positions do not move
    tg = g8.copy(); tg[2] = -1; tg[7] = -1
    a = gpu.RunState(cfg); a.prefill(toks[:5], 0, w)
    lp_a, top_a = a.score(t8, 5, w, targets=g8)
    b = gpu.RunState(cfg); b.prefill(toks[:5], 0, w)
    lp_b, top_b = b.score(t8, 5, w, targets=tg)
    assert lp_b[2] == 0.0 and lp_b[7] == 0.0 and not np.signbit(lp_b[[2, 7]]).any()
    keep = [0, 1, 3, 4, 5, 6]
    assert np.array_equal(lp_a[keep], lp_b[keep]) and np.array_equal(top_a, top_b) and (lp_a < 0).all()
    # out_top1 = NULL / targets = NULL: the other output, bit for bit
    c = gpu.RunState(cfg); c.prefill(toks[:5], 0, w)
    lp_c, none = c.score(t8, 5, w, targets=g8, top1=False)
    assert none is None and np.array_equal(lp_c, lp_a)
    d = gpu.RunState(cfg); d.prefill(toks[:5], 0, w)
    top_d = np.zeros(8, np.int32)
    assert call(t8, 8, 5, None, None, top_d, state=d) == gpu.OK
    assert np.array_equal(top_d, top_a)
    # the default call: next-token targets, none for the last
    e = gpu.RunState(cfg); e.prefill(toks[:5], 0, w)
    lp_e, top_e = e.score(t8, 5, w)
    assert np.array_equal(lp_e[:7], lp_a[:7]) and lp_e[7] == 0.0 and np.array_equal(top_e, top_a)
    for x in (a, b, c, d, e, s):
        x.close()
    w.close()


def test_same_bits_run_to_run_and_whatever_the_slab(gpu, ck, options):
    """Two identical calls on fresh runstates give identical bits; so does a run with the classifier product forced into
    eight slabs (the reduction's segments, not the slabs, fix the order of the sums), and one on a runstate whose
    workspace was sized by an earlier, longer call."""
    options(L2Z_PF_X3=1)
    cfg = ck.Config(**SMALL)
    w = gpu.Weights(cfg, None, False, seed=23)
    toks = case_tokens(cfg, 200)
    outs = []
    for slab in (0, 0, 4096, 12288):
        s = gpu.RunState(cfg)
        if slab:
            s.score_slab_set(slab)
        outs.append(s.score(toks, 0, w))
        s.close()
    for lp, top in outs[1:]:
        assert np.array_equal(lp, outs[0][0]) and np.array_equal(top, outs[0][1])
    s = gpu.RunState(cfg)
    s.score(case_tokens(cfg, 310), 0, w)
    lp, top = s.score(toks[:60], 0, w)
    s2 = gpu.RunState(cfg)
    lp2, top2 = s2.score(toks[:60], 0, w)
    assert np.array_equal(lp, lp2) and np.array_equal(top, top2)
    s.close(); s2.close(); w.close()


def encode(cfg, text):
    H = C.CDLL(os.path.join(HOST, "libllama2_host.so"))
    H.l2zh_tokenizer_open.restype = C.c_void_p
    H.l2zh_tokenizer_open.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    H.l2zh_tokenizer_close.argtypes = [C.c_void_p]
    H.l2zh_tokenizer_encode.restype = C.c_long
    H.l2zh_tokenizer_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int32), C.c_size_t]
    err = C.create_string_buffer(128)
    t = H.l2zh_tokenizer_open(TOK.encode(), cfg.vocab_size, err, 128)
    assert t, err.value
    out = (C.c_int32 * 256)()
    n = H.l2zh_tokenizer_encode(t, text.encode(), len(text.encode()), out, 256)
    H.l2zh_tokenizer_close(t)
    assert n >= 4
    return [int(v) for v in out[:n]]


LINE = re.compile(r'^(\d+)\t(\d+)\t"(.*)"\t(-?\d+\.\d{6})\t(\d+)$')
TEXT = "Once upon a time there was a little dog who liked to play in the park"


def run_score_cli(path, text):
    r = subprocess.run([EXE, path, "--score", "-z", TOK, "-i", text], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    rows = [LINE.match(ln) for ln in lines[:-3]]
    assert all(rows), r.stdout
    tail = dict(ln.split(": ") for ln in lines[-3:])
    return ([int(m.group(2)) for m in rows], np.array([float(m.group(4)) for m in rows]),
            [int(m.group(5)) for m in rows], tail)


@pytest.mark.parametrize("hidden", [768, 770], ids=["one-score-call", "stepped-fallback"])
def test_cli_score(gpu, ck, orc, options, tmp_path, hidden):
    """`llama2 ckpt --score -i text`: one line per prompt token, then the totals.  The printed log-probs are the
    binding's (hidden 768) or, for a width that is not a multiple of 4, the stepped fallback's -- both within the bar of
    the oracle; the perplexity is exp(-mean) of the printed values."""
    options(L2Z_PF_X3=1)
    cfg = ck.Config(**dict(SMALL, hidden_dim=hidden))
    blob = ck.synth_blob(cfg, True, seed=23)
    path = str(tmp_path / "toy.bin")
    ck.write_checkpoint(path, cfg, blob, True)
    prompt = encode(cfg, TEXT)
    ids, lps, tops, tail = run_score_cli(path, TEXT)
    assert ids == prompt and [int(tail["tokens"])] == [len(prompt)]
    nll = -lps.mean()
    assert abs(float(tail["nll/token"]) - nll) <= 1e-6 * max(1.0, abs(nll)) + 1e-6
    assert abs(float(tail["perplexity"]) / np.exp(nll) - 1.0) <= 1e-6
    inp = np.array([1] + prompt[:-1], np.int32)
    w, s = gpu.Weights(cfg, blob, True), gpu.RunState(cfg)
    if hidden % 4 == 0:
        lp, top = s.score(inp, 0, w, targets=np.array(prompt, np.int32))
        assert np.all(np.abs(lps - lp.astype(np.float64)) <= 5.1e-7 + 1e-7 * np.abs(lp))   # %.6f of the same f32 values
        assert tops == top.tolist()
    else:
        with pytest.raises(gpu.L2ZError) as e:
            s.score(inp, 0, w, targets=np.array(prompt, np.int32))
        assert e.value.code == gpu.ERR_INVALID
    s.close(); w.close()
    m = orc.Model(cfg.as_i32(), blob, True)
    for i, t in enumerate(inp):
        z = m.transformer(int(t), i).astype(np.float64)
        ref = z[prompt[i]] - (z.max() + np.log(np.exp(z - z.max()).sum()))
        bar = bar_of(np.abs(z).max())
        assert abs(lps[i] - ref) <= bar + 5e-7, (i, lps[i], ref)   # (+ the rounding of the printed value)
        two = np.partition(z, -2)[-2:]
        if two[1] - two[0] > bar:
            assert tops[i] == int(np.argmax(z))
    m.close()


def test_cli_score_refuses_a_prompt_longer_than_seq_len(gpu, ck, tmp_path):
    cfg = ck.Config(**dict(TOY, seq_len=8))
    path = str(tmp_path / "short.bin")
    ck.write_checkpoint(path, cfg, ck.synth_blob(cfg, False, seed=23), False)
    r = subprocess.run([EXE, path, "--score", "-z", TOK, "-i", TEXT], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "seq_len" in r.stderr and "tokens:" not in r.stdout
