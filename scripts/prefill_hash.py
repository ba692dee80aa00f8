"""One SHA-256 per case of the raw output bytes of the batched prompt pass: run it once per build of the library
(L2Z_LIB names the build, each run a process of its own) and diff the two outputs -- a refactor of the prefill GEMM kernels
must leave every line equal.  The prefill sibling of decode_hash.py.  A case is a one- or two-layer model of synthetic
weights, a chunk length and the knobs that send its products (q | k | v, Wo, W1 | W3, W2) to the kernel form the case is there
for; before a case is hashed its plan is asserted on the device's own CU count, so that no case silently moves to another
family.  The table (MODELS, CASES, products) imports without a device: tests/test_prefill_hash_cases.py checks what it reaches.

usage: L2Z_LIB=/path/to/libllama2_hip_test.so python scripts/prefill_hash.py > hashes.txt"""
import hashlib, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, __graft_entry__ as ge
pkg = ge.load_package(); B, ck = pkg.binding, pkg.checkpoint

# widths of: llama2-7b; the same with ONE kv head of 64 and a narrow hidden layer (q | k | v and W1 | W3 block-starved at 100
# tokens: two K ranges); 63 heads of 64 (no 128-feature tiles of a fused q | k | v: q, k, v apart on 128 x 128 tiles); a hidden
# layer whose W1 | W3 launch does not fit one round of blocks; tests/test_gpu_x3.py's wide model; stories15M (K = 288 is
# walked as 320)
MODELS = {
    "7b": dict(dim=4096, hidden_dim=11008, n_layers=1, n_heads=32, n_kv_heads=32, vocab_size=1000, seq_len=1024),
    "gqa": dict(dim=4096, hidden_dim=5632, n_layers=1, n_heads=64, n_kv_heads=1, vocab_size=1000, seq_len=128),
    "63h": dict(dim=4032, hidden_dim=5632, n_layers=1, n_heads=63, n_kv_heads=63, vocab_size=1000, seq_len=1024),
    "wide": dict(dim=4096, hidden_dim=19200, n_layers=1, n_heads=32, n_kv_heads=32, vocab_size=1000, seq_len=128),
    "2k": dict(dim=2048, hidden_dim=14336, n_layers=1, n_heads=16, n_kv_heads=16, vocab_size=1000, seq_len=128),
    "15m": dict(dim=288, hidden_dim=768, n_layers=2, n_heads=6, n_kv_heads=6, vocab_size=1000, seq_len=128),
}
DEFAULTS = {"L2Z_PF_X3": 1, "L2Z_PF_X3_STREAM_MIN": 33, "L2Z_PF_PANEL": 1, "L2Z_PF_PANEL_MAX": -1, "L2Z_PF_CHUNK": 0, "L2Z_PF_FUSE_PLANES": 1}
F32 = {"L2Z_PF_X3": 0}                          # the f32 matrix cores
F32_NO_PANEL = {"L2Z_PF_X3": 0, "L2Z_PF_PANEL": 0}   # ... and chunks of 17 ... 96 tokens to the short-prompt / tile kernels
STORE, RESID, ROPE, ROPE_CACHE, CACHE, SWIGLU = range(6)   # PrefillGemmEpi


def products(m, P):
    """The products of one layer of model m at a chunk of P tokens and the plan of each, as prefill_host.cpp launches them
    (prefill_stage, launch_qkv, launch_w13) when the panel kernel does not take the chunk: {name: l2z_prefill_gemm_plan}."""
    dim, hid = m["dim"], m["hidden_dim"]
    kvd = dim // m["n_heads"] * m["n_kv_heads"]
    n_qkv, r64 = dim + 2 * kvd, lambda k: (k + 63) // 64 * 64
    sk_qkv, sk_wo = B.prefill_split_k(n_qkv, P, r64(dim)), B.prefill_split_k(dim, P, r64(dim))
    sk_w2, sk_h1 = B.prefill_split_k(dim, P, r64(hid)), B.prefill_split_k(hid, P, r64(dim), True)
    plan, out = B.prefill_gemm_plan, {}
    qkv = plan("qkv", P, n_qkv, dim, nq=dim, nkv=kvd, sk=sk_qkv)
    if qkv["family"] != "not supported":
        out["qkv"] = qkv
    else:   # q, then k | v paired (short prompts), else k and v
        out["q"] = plan("single", P, dim, dim, epi=ROPE, sk=sk_qkv, n_launch_whole=n_qkv)
        kv = plan("kv", P, kvd, dim, sk=sk_qkv, n_launch_whole=n_qkv)
        if kv["family"] != "not supported":
            out["kv"] = kv
        else:
            out["k"] = plan("single", P, kvd, dim, epi=ROPE_CACHE, sk=sk_qkv, n_launch_whole=n_qkv)
            out["v"] = plan("single", P, kvd, dim, epi=CACHE, sk=sk_qkv, n_launch_whole=n_qkv)
    out["wo"] = plan("single", P, dim, dim, epi=RESID, sk=sk_wo)
    w13 = plan("w13", P, hid, dim, w13_one_matrix=1, sk=sk_h1)
    if w13["family"] != "not supported":
        out["w13"] = w13
    else:
        out["w1"] = plan("single", P, hid, dim, epi=STORE, sk=sk_h1)
        out["w3"] = plan("single", P, hid, dim, epi=SWIGLU, sk=sk_h1)
    out["w2"] = plan("single", P, dim, hid, epi=RESID, sk=sk_w2)
    return out


def takes_panel(m, P):
    """Whether the model's Wo takes the K-range panel kernel at P tokens (under the options set) -- an INDIRECT witness, the only
    one there is without a hook into prefill_panel_shape: the chunk planner cuts a tail of 128 + 32 tokens in two exactly where
    32 tokens take the kernel, and -- were the kernel's longest chunk 64 tokens (L2Z_PF_PANEL_MAX) -- a tail of 80 tokens into
    48 + 32 exactly where both do.  True / False at 32 and 48 tokens; None at every other length: NOT ANSWERED.  (There the
    table's own rule stands in: tests/test_prefill_hash_cases.py wants the panel kernel switched off in every case whose
    chunk it could take.)"""
    cfg = ck.Config(**m)
    if P == 32:
        return B.prefill_plan(160, cfg) == [128, 32]
    if P != 48:
        return None
    B.option_set("L2Z_PF_PANEL_MAX", 64)
    try:
        return B.prefill_plan(80, cfg) == [48, 32]
    finally:
        B.option_set("L2Z_PF_PANEL_MAX", DEFAULTS["L2Z_PF_PANEL_MAX"])


# (name, model, tokens, options, {product: the plan fields the case is there for})
T = lambda tile, **kw: dict(family="tile", tile=tile, **kw)
SK = lambda sk, **kw: dict(family="split-k", sk=sk, x3=0, **kw)
TWO = lambda tile: dict(family="two-block", tile=tile, x3=0)
ST = lambda feat, sk, tm, **kw: dict(family="stream", x3=1, feat=feat, sk=sk, tm=tm, **kw)
SHORT = lambda tms, paired=0: dict(family="short", tms=tms, paired=paired)
CASES = [
    # the tile kernel on the f32 cores, every tile form (32 x 32: a cache-resident model; K = 288 walked as 320)
    ("7b f32 1024", "7b", 1024, F32, {"qkv": TWO("128x128"), "wo": TWO("128x128"), "w13": TWO("128x64"), "w2": TWO("128x128")}),
    ("63h f32 1024", "63h", 1024, F32, {"q": T("128x128", x3=0), "k": T("128x128", x3=0), "v": T("128x128", x3=0)}),
    ("7b f32 512", "7b", 512, F32, {"qkv": TWO("128x64"), "wo": TWO("128x64"), "w13": TWO("128x64"), "w2": TWO("128x64")}),
    ("7b f32 500", "7b", 500, F32, {"q": T("128x64", x3=0), "k": T("128x64", x3=0), "v": T("128x64", x3=0), "wo": T("128x64", x3=0),
                                   "w13": T("128x64", x3=0), "w2": T("128x64", x3=0)}),
    ("7b f32 256", "7b", 256, F32, {"qkv": T("64x64", x3=0, epi=6), "wo": T("64x64", x3=0), "w13": T("64x64", x3=0)}),
    ("7b f32 100", "7b", 100, F32, {"qkv": T("32x64", x3=0, epi=6), "w13": T("32x64", x3=0), "wo": SK(2, tile="64x64"), "w2": SK(2, k=11008)}),
    ("15m 100", "15m", 100, {}, {"qkv": T("32x32", x3=0, k=320, epi=6), "wo": T("32x32", x3=0, k=320), "w13": T("32x32", x3=0, k=320),
                                 "w2": T("32x32", x3=0, k=768)}),
    # ... and on the bf16 cores
    ("7b bf16 1024", "7b", 1024, {}, {"q": T("128x128", x3=1), "wo": T("128x128", x3=1), "w13": T("128x64", x3=1, epi=0)}),
    ("7b bf16 512", "7b", 512, {}, {"q": T("128x64", x3=1), "w13": T("128x64", x3=1, epi=0), "w2": T("128x64", x3=1)}),
    ("7b bf16 256", "7b", 256, {}, {"qkv": T("64x64", x3=1, epi=6), "wo": T("64x64", x3=1)}),
    # split-K: four ranges at 64 tokens, two at 100 -- the residual products, the pair, q | k | v fused
    ("7b f32 64 split-k", "7b", 64, F32_NO_PANEL, {"qkv": SK(4, epi=6), "wo": SK(4), "w13": SK(4, epi=0), "w2": SK(4)}),
    ("gqa f32 100 split-k", "gqa", 100, F32, {"qkv": SK(2, epi=6), "wo": SK(2), "w13": SK(2, epi=0), "w2": SK(2)}),
    # the stream form: 128 / 192 / 256 features per block, two and four token tiles, 2 / 4 / 8 ranges
    ("7b bf16 64 stream", "7b", 64, {}, {"qkv": ST(192, 4, 2, epi=6, one_round=1), "wo": ST(128, 8, 2, one_round=1),
                                         "w13": ST(192, 2, 2, epi=7, one_round=1), "w2": ST(128, 8, 2, one_round=1)}),
    ("7b bf16 100 stream", "7b", 100, {}, {"qkv": ST(128, 2, 4, epi=6), "wo": ST(128, 8, 4, nbuf=4, one_round=1), "w2": ST(128, 8, 4)}),
    ("7b bf16 128 stream", "7b", 128, {}, {"qkv": ST(128, 2, 4, epi=6), "wo": ST(128, 8, 4)}),
    ("2k bf16 40 stream", "2k", 40, {}, {"qkv": ST(192, 8, 2, epi=6, nbuf=4, one_round=1), "wo": SHORT(1), "w13": ST(256, 2, 2, epi=7, nbuf=3, one_round=1),
                                         "w2": ST(128, 8, 2, nbuf=5, one_round=1)}),
    # ... a launch of several rounds of blocks: the last arriver of a tile adds the ranges (one_round 0, more than one range)
    ("wide bf16 100 stream, several rounds", "wide", 100, {}, {"w13": ST(128, 2, 4, epi=7, one_round=0)}),
    # the short-prompt kernels: one and two token tiles of 16, paired (W1 | W3, k | v)
    ("7b f32 16 short", "7b", 16, F32_NO_PANEL, {"q": SHORT(1), "kv": SHORT(1, 1), "wo": SHORT(1), "w13": SHORT(1, 1), "w2": SHORT(1)}),
    ("7b f32 24 short", "7b", 24, F32_NO_PANEL, {"q": SHORT(2), "k": SHORT(2), "v": SHORT(2), "wo": SHORT(2), "w1": SHORT(2), "w3": SHORT(2), "w2": SHORT(2)}),
    ("15m 40 short", "15m", 40, {}, {"q": SHORT(1), "wo": SHORT(1)}),
    # the K-range panel kernel (takes_panel; its products go through launch_prefill_panel, not through the plans)
    ("7b 32 panel", "7b", 32, {}, "panel"),
    ("7b f32 48 panel", "7b", 48, F32, "panel"),
]


def check_case(case):
    """Asserts that the case's products take the forms it names, under its options (set and put back here)."""
    name, model, P, opts, want = case
    m = MODELS[model]
    for k, v in opts.items():
        B.option_set(k, v)
    try:
        assert B.prefill_plan(P, ck.Config(**m)) == [P], (name, B.prefill_plan(P, ck.Config(**m)))   # one chunk
        if want == "panel":
            assert takes_panel(m, P) is True, name   # (a panel case sits at a length the witness answers)
            return
        assert takes_panel(m, P) is not True, name   # (says something at 32 and 48 tokens only: see takes_panel)
        got = products(m, P)
        for prod, fields in want.items():
            assert prod in got, (name, prod, sorted(got))
            bad = {f: (got[prod][f], v) for f, v in fields.items() if got[prod][f] != v}
            assert not bad, (name, prod, bad)
    finally:
        for k in opts:
            B.option_set(k, DEFAULTS[k])


def emit(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(f"{h.hexdigest()}  {name}", flush=True)


def caches(s, cfg, kvd=None):
    """every layer's whole key and value cache (rows past the prompt included: nothing may land there)"""
    n = cfg.n_layers * cfg.seq_len * (kvd or cfg.kv_dim)
    return [s.read(nm, 0, n) for nm in ("key_cache", "value_cache")]


def tokens(cfg, n, seed=1):
    return np.array([1] + np.random.default_rng(seed).integers(2, cfg.vocab_size, n - 1).tolist(), np.int32)


def main():
    for k, v in DEFAULTS.items():
        B.option_set(k, v)
    weights = {}
    W = lambda model: weights.setdefault(model, B.Weights(ck.Config(**MODELS[model]), None, False, seed=77))
    for case in CASES:
        name, model, P, opts, _ = case
        check_case(case)
        cfg = ck.Config(**MODELS[model])
        for k, v in opts.items():
            B.option_set(k, v)
        s = B.RunState(cfg)
        s.prefill(tokens(cfg, P), 0, W(model))
        emit(f"prefill {name}: logits, K / V caches", s.logits(), *caches(s, cfg))
        s.close()
        for k in opts:
            B.option_set(k, DEFAULTS[k])
    small, w = ck.Config(**MODELS["15m"]), W("15m")   # (stays for the cases below)
    for model, wt in weights.items():
        if model != "15m":
            wt.close()
    # two emulated ranks under each sharding scheme: rows (A), Wo / W2 by columns (B)
    for scheme_b in (0, 1):
        B.option_set("L2Z_SCHEME_B", scheme_b)
        try:
            comms = [B.Comm(r, 2, None, 0, emulated=True) for r in range(2)]
            ws = [B.Weights(small, None, False, seed=77, comm=c) for c in comms]
            ss = [B.RunState(small, comm=c) for c in comms]
        finally:
            B.option_set("L2Z_SCHEME_B", 0)
        B.emu_prefill(ss, ws, tokens(small, 100), 0)
        emit(f"emu_prefill 15m 100 tokens, 2 ranks, scheme {'B' if scheme_b else 'A'}: logits, K / V caches of both ranks",
             *[a for s in ss for a in [s.logits()] + caches(s, small, small.kv_dim // 2)])
        for o in ss + ws + comms:
            o.close()
    # rows of several sequences in one pass
    ss = [B.RunState(small) for _ in range(3)]
    B.prefill_batch(ss, [tokens(small, n, seed=n) for n in (5, 40, 19)], [0, 0, 0], w)
    emit("prefill_batch 15m 5 / 40 / 19 rows: logits, K / V caches of each", *[a for s in ss for a in [s.logits()] + caches(s, small)])
    for s in ss:
        s.close()
    # every row's logits reduced; the classifier product
    s = B.RunState(small)
    lp, top = s.score(tokens(small, 100), 0, w)
    emit("score 15m 100 tokens: log-probs, top-1 ids, logits, K / V caches", lp, top, s.logits(), *caches(s, small))
    s.close()
    # a sequence's token and seven guesses: the short-prompt kernel with the per-row epilogues
    s = B.RunState(small)
    s.prefill(tokens(small, 20), 0, w)
    nxt, acc = s.verify(tokens(small, 8, seed=3), 20, w)
    emit("verify 15m 8 rows at position 20: next ids, accepted, every row's logits, K / V caches", nxt, np.array([acc], np.int32),
         *[s.verify_logits(r) for r in range(8)], *caches(s, small))
    s.close()
    w.close()


if __name__ == "__main__":
    main()
