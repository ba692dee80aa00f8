"""One SHA-256 per case of the raw output bytes of the single-token decode path: run it once per build of the library
(L2Z_LIB names the build, each run a process of its own) and diff the two outputs -- a refactor of the decode kernels
must leave every line equal.  The cases are the shapes at which each kernel form can still go wrong; a few seconds in all.

usage: L2Z_LIB=/path/to/libllama2_hip_test.so python scripts/decode_hash.py > hashes.txt"""
import hashlib, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np, __graft_entry__ as ge
pkg = ge.load_package(); B, ck = pkg.binding, pkg.checkpoint


def emit(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(f"{h.hexdigest()}  {name}", flush=True)


rng = np.random.default_rng(2025)
# mat-vec: scalar kernel, LPR 8 / 16 / 32 / 64, a partial last step, the row kernel with XC 4 and 12, odd row counts
for d, n in ((3, 3), (2, 12), (7, 5), (33, 172), (33, 64), (33, 288), (33, 512), (33, 768), (33, 1376), (34, 4096), (33, 11008)):
    x, w = rng.standard_normal(n, dtype=np.float32), rng.standard_normal((d, n), dtype=np.float32)
    emit(f"matmul d={d} n={n}", B.matmul(x, w))
# fused segments; odd rows per segment, so a pair straddles every segment boundary
for N in (2, 3):
    for d, n in ((33, 288), (5, 4096)):
        x = rng.standard_normal(n, dtype=np.float32)
        ws = [rng.standard_normal((d, n), dtype=np.float32) for _ in range(N)]
        emit(f"matmul_fused N={N} d={d} n={n}", *B.matmul_fused(x, ws))


def kv_rows(s, cfg, n_pos, kvd=None):
    kvd = kvd or cfg.kv_dim
    return [s.read(nm, l * cfg.seq_len * kvd, n_pos * kvd) for nm in ("key_cache", "value_cache") for l in range(cfg.n_layers)]


def greedy(name, cfg, steps=8, sample=False, **opts):
    """steps forward passes fed with their own argmax (logits of each), then the same steps as one greedy run (the
    captured step: fused classifier argmax, argmax_kernel's hand-over), and the K / V rows both wrote"""
    for k, v in opts.items():
        B.option_set(k, v)
    w, s = B.Weights(cfg, None, False, seed=77), B.RunState(cfg)
    tok, lgs, ids = 1, [], []
    for pos in range(steps):
        s.transformer(tok, pos, w)
        lgs.append(s.logits())
        tok = s.argmax()
        ids.append(tok)
    emit(f"{name}: logits of {steps} steps", *lgs)
    emit(f"{name}: argmax ids", np.array(ids, np.int32))
    emit(f"{name}: K / V rows", *kv_rows(s, cfg, steps))
    s2 = B.RunState(cfg)
    s2.greedy_begin([])
    emit(f"{name}: greedy_run ids", s2.greedy_run(w, steps))
    emit(f"{name}: greedy_run logits, K / V rows", s2.logits(), *kv_rows(s2, cfg, steps))
    if sample:
        sample_run(name, cfg, w, steps)
    for o in (s, s2, w):
        o.close()


def sample_run(name, cfg, w, steps=8):
    """the sampled loop: the same pass with the draw as its last node"""
    s = B.RunState(cfg)
    s.greedy_begin([3, 4])
    coins = np.random.default_rng(7).random(steps, dtype=np.float32)
    emit(f"{name}: sample_run ids, logits", s.sample_run(w, steps, 0.9, 0.95, coins), s.logits())
    s.close()


small = ck.Config(dim=288, hidden_dim=768, n_layers=2, n_heads=6, n_kv_heads=6, vocab_size=1000, seq_len=64)
big = ck.Config(dim=4096, hidden_dim=11008, n_layers=1, n_heads=32, n_kv_heads=32, vocab_size=1000, seq_len=64)
greedy("dim 288", small)
greedy("dim 288, per-kernel launches", small, L2Z_FUSE_SMALL=0)
B.option_set("L2Z_FUSE_SMALL", 1)
greedy("dim 4096 packed", big, L2Z_PACKED_W=1)
greedy("dim 4096 f32", big, L2Z_PACKED_W=0)
B.option_set("L2Z_PACKED_W", 1)
# ... and the packed copy in each form it can be built and attached: 28 / 29 bits, the kinds that may take 28 (the
# default 40 = ffn13 | cls, then every kind), every single kind's launches alone on the copy (qkv 1, wo 4, ffn13 8, ffn2 16, cls 32)
for bits, kinds28 in ((29, 40), (28, 40), (28, 63)):
    greedy(f"dim 4096 packed, bits {bits}, 28-bit kinds {kinds28}", big, sample=True, L2Z_PACKED_BITS=bits, L2Z_PACKED28_KINDS=kinds28)
B.option_set("L2Z_PACKED_BITS", 28)
B.option_set("L2Z_PACKED28_KINDS", 40)
for bit in (1, 4, 8, 16, 32):
    greedy(f"dim 4096 packed, kinds mask {bit}", big, steps=4, L2Z_PACKED_KINDS=bit)
B.option_set("L2Z_PACKED_KINDS", -1)

# int8 group-quantized weights (tests/q8_cases.py: an MHA shape whose runstate has the fused small-model form set, and
# the shape that takes both loops of the kernel): the stepped pass, the greedy loop, the sampled loop
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import q8_cases  # noqa: E402
for qname in ("288", "tall"):
    cfg, gs, _, body = q8_cases.model(qname)
    w = B.Weights.from_q8(cfg, body, True, gs)
    s = B.RunState(cfg)
    tok, lgs, ids = 1, [], []
    for pos in range(8):
        s.transformer(tok, pos, w)
        lgs.append(s.logits())
        tok = s.argmax()
        ids.append(tok)
    emit(f"q8 {qname}: logits of 8 steps, argmax ids", *lgs, np.array(ids, np.int32))
    emit(f"q8 {qname}: K / V rows", *kv_rows(s, cfg, 8))
    s2 = B.RunState(cfg)
    s2.greedy_begin([])
    emit(f"q8 {qname}: greedy_run ids", s2.greedy_run(w, 8))
    emit(f"q8 {qname}: greedy_run last logits, K / V rows", s2.logits(), *kv_rows(s2, cfg, 8))
    sample_run(f"q8 {qname}", cfg, w)
    for o in (s, s2, w):
        o.close()

# two emulated ranks of the small model on one GPU
comms = [B.Comm(r, 2, None, 0, emulated=True) for r in range(2)]
ws = [B.Weights(small, None, False, seed=77, comm=c) for c in comms]
ss = [B.RunState(small, comm=c) for c in comms]
tok, out = 1, []
for pos in range(8):
    B.emu_transformer(ss, ws, tok, pos)
    out += [s.logits() for s in ss]
    tok = ss[0].argmax()
emit("dim 288, 2 emulated ranks: logits of 8 steps, both ranks", *out)
emit("dim 288, 2 emulated ranks: K / V rows", *[a for s in ss for a in kv_rows(s, small, 8, small.kv_dim // 2)])
for o in ss + ws + comms:
    o.close()

# rank 0 of 2 alone, hand-overs free: the LL consume and push forms of the mat-vec and attention kernels (the numbers
# mean nothing -- the peer's slices read as zeros -- but they are a function of the kernels alone)
for consume in (1, 0):
    B.option_set("L2Z_P2P_CONSUME", consume)
    B.option_set("L2Z_P2P_TIMEOUT_S", 5)
    try:
        comm = B.Comm(0, 2, None, 0)
        comm.p2p_export(max(small.dim, small.hidden_dim, small.vocab_size, 2 * small.dim), max(small.dim, small.hidden_dim))
        comm.p2p_connect_solo()
        w, s = B.Weights(small, None, False, seed=77, comm=comm), B.RunState(small, comm=comm)
    finally:
        B.option_set("L2Z_P2P_CONSUME", -1)
        B.option_set("L2Z_P2P_TIMEOUT_S", 20)
    s.greedy_begin([5, 6])
    emit(f"dim 288, solo rank 0 of 2, consume {consume}: greedy ids, logits", s.greedy_run(w, 8), s.logits())
    s.close(); w.close(); comm.close()

# decode attention, every form
for hs in (11, 48, 64, 128):
    n_heads, n_kv = 4, 2
    for S in (512, 2048):
        q = rng.standard_normal(n_heads * hs, dtype=np.float32)
        kc = rng.standard_normal(S * n_kv * hs, dtype=np.float32)
        vc = rng.standard_normal(S * n_kv * hs, dtype=np.float32)
        forms = [("generic", 0)] if hs == 11 else [("auto", 0), ("fast256", 0), ("fast1024", 0), ("generic", 0), ("split", 2), ("split", 3), ("split", 8)]
        for form, nch in forms:
            outs = [B.attention_decode(q, kc, vc, pos, n_heads, n_kv, hs, S, form, nch) for pos in (0, 1, 63, 64, 255, 300, S - 1)]
            emit(f"attention hs={hs} seq_len={S} {form} nch={nch}", *outs)
