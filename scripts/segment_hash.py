"""One SHA-256 per case of the raw output bytes of everything that runs on the segment attention (verify_device.h): the wide
step and its run, the chain, batch and tree verify.  Run it once per build of the library (L2Z_LIB names the build, each run
a process of its own) and diff the two outputs -- a refactor of the segment bodies must leave every line equal.  The models
are synthetic, one or two layers, seq_len 192 (three segments); head sizes 8, 48, 64, 128, 256 (2, 16 with idle lanes, 16,
32, 64 lanes per K row) and 1, 2, 3, 4, 6, 8 query heads per kv head.  Well under a minute.

usage: L2Z_LIB=/path/to/libllama2_hip_test.so python scripts/segment_hash.py > hashes.txt"""
import hashlib, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, __graft_entry__ as ge
pkg = ge.load_package(); B, ck = pkg.binding, pkg.checkpoint

L = 192
EDGES = [0, 1, 63, 64, 65, 127, 128, 191]


def emit(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(f"{h.hexdigest()}  {name}", flush=True)


def kv_rows(s, cfg, lo, hi):
    """rows lo .. hi - 1 of every kv head of every layer of both caches (head-major: [layer][kv head][seq_len][head_size])"""
    hs, nkv = cfg.dim // cfg.n_heads, cfg.n_kv_heads
    return [s.read(nm, ((l * nkv + h) * cfg.seq_len + lo) * hs, (hi - lo) * hs)
            for nm in ("key_cache", "value_cache") for l in range(cfg.n_layers) for h in range(nkv)]


def forked(base, depth):
    s = B.RunState(base.cfg)
    B.runstate_fork(s, base, depth)
    s.synchronize()
    return s


class Model:
    def __init__(self, name, dim, hidden, heads, kv, layers=1, vocab=512):
        self.name = f"{name} hs={dim // heads} kv_mul={heads // kv}"
        self.cfg = ck.Config(dim=dim, hidden_dim=hidden, n_layers=layers, n_heads=heads, n_kv_heads=kv, vocab_size=vocab, seq_len=L)
        self.rng = np.random.default_rng([2026, dim, heads, kv])
        self.w = B.Weights(self.cfg, None, False, seed=91)
        self.prefix = np.array([1] + self.rng.integers(2, vocab, L - 2).tolist(), np.int32)
        self.base = B.RunState(self.cfg)
        self.base.prefill(self.prefix, 0, self.w)

    def close(self):
        self.base.close()
        self.w.close()

    def wide(self, n=33, tag=""):
        cfg, rng = self.cfg, self.rng
        pos = np.array(EDGES + rng.integers(0, L, n - len(EDGES)).tolist(), np.int32)
        tok = rng.integers(2, cfg.vocab_size, n).astype(np.int32)
        ss = [forked(self.base, int(p)) for p in pos]
        nxt = B.transformer_wide(ss, tok, pos, self.w)
        emit(f"{self.name}: wide step n={n}{tag}: next, logits", nxt, *[s.logits() for s in ss])
        emit(f"{self.name}: wide step n={n}{tag}: K / V rows", *[a for s, p in zip(ss, pos) for a in kv_rows(s, cfg, int(p), int(p) + 1)])
        for s in ss:
            s.close()

    def wide_run(self, n=33, steps=3):
        cfg, rng = self.cfg, self.rng
        pos = np.minimum(np.array(EDGES + rng.integers(0, L, n - len(EDGES)).tolist(), np.int32), L - steps)
        tok = rng.integers(2, cfg.vocab_size, n).astype(np.int32)
        temp = np.where(np.arange(n) % 3 == 0, 0.0, 0.9).astype(np.float32)
        coins = rng.random((steps, n), dtype=np.float32)
        for tag, kw in (("greedy", {}), ("sampled", dict(temperature=temp, top_p=0.9, coins=coins))):
            ss = [forked(self.base, int(p)) for p in pos]
            ids = B.wide_run(ss, tok, pos, self.w, steps, **kw)
            emit(f"{self.name}: wide_run {tag} n={n} steps={steps}: ids, final logits", ids, *[s.logits() for s in ss])
            for s in ss:
                s.close()

    def guesses(self, n):
        return self.rng.integers(2, self.cfg.vocab_size, n).astype(np.int32)

    def chain(self):
        cfg = self.cfg
        for pos0 in (0, 60, 120):
            for n in (1, 8, 16):
                t = self.guesses(n)
                if pos0 == 0:
                    t[0] = 1
                for tag, sample in (("greedy", None), ("sampled", (0.9, 0.9, self.rng.random(n, dtype=np.float32)))):
                    for rnd in (0, 1):   # the second pass guesses the first's own next ids for half of its rows: accepted > 0
                        s = forked(self.base, pos0)
                        nxt, acc = s.verify(t, pos0, self.w) if sample is None else s.verify_sample(t, pos0, self.w, *sample)
                        emit(f"{self.name}: verify {tag} pos0={pos0} n={n} pass {rnd}: next, accepted, rows' logits, K / V rows, logits",
                             nxt, np.int32(acc), *[s.verify_logits(i) for i in range(n)], *kv_rows(s, cfg, pos0, pos0 + n), s.logits())
                        s.close()
                        t = t.copy()
                        t[1:1 + n // 2] = nxt[:n // 2]

    def batch(self):
        cfg = self.cfg
        pos0s = [0, 60, 120, 17]
        lens = [5, 6, 4, 1]   # 16 rows: groups of unequal length and depth; two straddle a segment boundary
        lists = [self.guesses(m) for m in lens]
        lists[0][0] = 1
        temp = np.array([0.0, 0.9, 0.7, 0.9], np.float32)
        coin_lists = [self.rng.random(m, dtype=np.float32) for m in lens]
        for tag, kw in (("greedy", {}), ("sampled", dict(temperature=temp, top_p=0.9, coin_lists=coin_lists))):
            ss = [forked(self.base, p) for p in pos0s]
            nxt, acc = B.verify_batch(ss, lists, pos0s, self.w, **kw)
            emit(f"{self.name}: verify_batch {tag}: next, accepted, rows' logits, K / V rows, logits", *nxt, acc,
                 *[ss[0].verify_logits(i) for i in range(sum(lens))],
                 *[a for s, p, m in zip(ss, pos0s, lens) for a in kv_rows(s, cfg, p, p + m)], *[s.logits() for s in ss])
            for s in ss:
                s.close()

    def tree(self, pos0=58):
        # 16 nodes, branching, depth 7: positions 58 .. 65 cross the boundary at 64
        parent = np.array([-1, 0, 0, 1, 1, 2, 3, 3, 4, 6, 6, 9, 9, 11, 11, 13], np.int32)
        t = self.guesses(16)
        for tag, kw in (("greedy", {}), ("sampled", dict(temperature=0.9, top_p=0.9, coins=self.rng.random(16, dtype=np.float32)))):
            s = forked(self.base, pos0)
            nxt, path, acc = s.verify_tree(t, parent, pos0, self.w, **kw)
            emit(f"{self.name}: verify_tree {tag} pos0={pos0}: next, path, accepted, rows' logits, K / V rows, logits", nxt, path,
                 np.int32(acc), *[s.verify_logits(i) for i in range(16)], *kv_rows(s, self.cfg, pos0, pos0 + 16), s.logits())
            s.close()


# (dim, hidden, heads, kv heads, layers): every head size's lane count, every kv_mul on both sides of the wide kernel's parts
MODELS = [("hs8", 64, 172, 8, 8, 2), ("hs8", 64, 172, 8, 4, 1), ("hs8", 64, 172, 8, 1, 1),
          ("hs48", 288, 768, 6, 6, 2), ("hs48", 288, 768, 6, 3, 1), ("hs48", 288, 768, 6, 2, 1), ("hs48", 288, 768, 6, 1, 2),
          ("hs64", 512, 1408, 8, 2, 1), ("hs64", 512, 1408, 8, 1, 1),
          ("hs128", 512, 1408, 4, 4, 1), ("hs128", 512, 1408, 4, 1, 2),
          ("hs256", 512, 1408, 2, 1, 1)]
for name, dim, hidden, heads, kv, layers in MODELS:
    m = Model(name, dim, hidden, heads, kv, layers)
    m.wide()
    m.wide_run()
    m.chain()
    m.batch()
    m.tree()
    m.close()

# a shape whose Wo runs on the bf16 cores: the wide combine writes the planes of bf16 terms (L2Z_PF_X3 1 and 2)
m = Model("bf16 cores", 3072, 8192, 24, 8, 1, vocab=1024)
assert all(B.prefill_gemm_plan("single", n, 3072, 3072)["x3"] for n in (33, 128))
for x3 in (1, 2):
    B.option_set("L2Z_PF_X3", x3)
    m.wide(33, f" x3={x3}")
    m.wide(128, f" x3={x3}")
B.option_set("L2Z_PF_X3", 1)
m.close()
