"""Packed against f32, kind by kind: l2z_time_kind on an f32 runstate (L2Z_PACKED_W=0) and a packed
runstate of ONE weights object, interleaved, five readings each; the rule of 4.9 -- a kind keeps the packed form only if
all five packed readings lie below all five f32 readings -- and the byte model beside it (3.8 us + bytes / 7.3 TB/s).
With a measurement build (scripts/timeline_build.sh, L2Z_LIB) also the row kernel's in-kernel stamps per kind and form.
usage: packed_kinds_ab.py [workload] [pos]"""
import ctypes as C, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, __graft_entry__ as ge
pkg = ge.load_package(); B, ck = pkg.binding, pkg.checkpoint
wl = sys.argv[1] if len(sys.argv) > 1 else "llama2-7b"
pos = int(sys.argv[2]) if len(sys.argv) > 2 else 0
cfg, shared = {n: (c, sh) for n, c, sh in ck.iter_configs()}[wl]
L = B.lib()
t0 = time.perf_counter(); w = B.Weights(cfg, None, shared, seed=2024); t_init = time.perf_counter() - t0
B.option_set("L2Z_PACKED_W", 0)
t0 = time.perf_counter(); w0 = B.Weights(cfg, None, shared, seed=2024); t_init0 = time.perf_counter() - t0
w0.close()
s_f = B.RunState(cfg)
B.option_set("L2Z_PACKED_W", 1)
s_p = B.RunState(cfg)
print(f"# {wl}: weights init {t_init0:.2f} s without the packed copy, {t_init:.2f} s with it")
KINDS = ["qkv", "wo", "ffn13", "ffn2", "cls"]
if hasattr(L, "l2z_weights_packed_count_kind"):
    L.l2z_weights_packed_count_kind.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
for k in KINDS if hasattr(L, "l2z_weights_packed_count_kind") else []:
    a, b = C.c_int(0), C.c_int(0)
    assert L.l2z_weights_packed_count_kind(w.h, B.KINDS.index(k), C.byref(a), C.byref(b)) == 0
    print(f"# {k}: {a.value} of {b.value} slots packed")
for p in (0, 1, 2):
    s_f.transformer(1 + p, p, w); lf = s_f.logits().view(np.uint32).copy()
    s_p.transformer(1 + p, p, w); lp = s_p.logits().view(np.uint32).copy()
    print(f"pos {p} logits bit-identical: {bool(np.array_equal(lf, lp))}")
d, h, v = cfg.dim, cfg.hidden_dim, cfg.vocab_size
kvd = d // cfg.n_heads * cfg.n_kv_heads
f32_bytes = {"qkv": 4 * d * (d + 2 * kvd), "wo": 4 * d * d, "ffn13": 8 * h * d, "ffn2": 4 * d * h, "cls": 4 * v * d}
ratio = {k: 0.90625 for k in KINDS}
if h % 1024:  # partial last batch of W2's rows: the in-row steps only
    full, rest = divmod(h // 4, 1024)
    steps = [sum(1 for q in range(4) if 64 * wv + 256 * q < rest) for wv in range(4)]
    ratio["ffn2"] = (full * 4 * 64 * 29 + sum(64 * ((29 * s_ + 3) // 4) for s_ in steps)) * 4 / (h * 8)
tl = hasattr(L, "l2z_matvec_timeline_dump")
NS, NB = 256, 512
def stamps(n_last):
    buf = (C.c_longlong * (NS * NB * 8))(); n = C.c_ulonglong(0)
    assert L.l2z_matvec_timeline_dump(buf, C.byref(n)) == 0
    t = np.frombuffer(buf, dtype=np.int64).reshape(NS, NB, 8)
    rows = []
    for i in range(n.value - n_last, n.value):
        r = t[i % NS]; r = r[r[:, 6] > 0]
        r = r[r[:, 0] > np.median(r[:, 0]) - 100000].astype(np.float64)  # (a slot keeps an earlier, wider launch's blocks)
        z = r[:, 0].min()
        rel = (r[:, :6] - z) / 100.0
        per_unit = r[:, 6] / r[:, 7]
        steady = (r[:, 4] - r[:, 3]) / 100.0 / np.maximum(r[:, 6] - per_unit, 1)
        rows.append([len(r)] + [f(rel[:, j]) for j in range(6) for f in (np.median, np.max)] + [np.median(steady), np.max(steady), np.median(r[:, 6])])
    return np.array(rows).mean(axis=0)
print("\n| kind | f32 us | packed us | ratio | model: 3.8 + packed bytes / 7.3 TB/s | share of the byte saving kept | all 5 packed < all 5 f32 | f32 readings | packed readings |\n|---|---:|---:|---:|---:|---:|---|---|---|")
tl_rows = []
for k in KINDS:
    rf, rp = [], []
    for _ in range(5):
        rf.append(s_f.time_kind(k, pos, w, reps=4)[0] * 1e3)
        rp.append(s_p.time_kind(k, pos, w, reps=4)[0] * 1e3)
    mf, mp = float(np.median(rf)), float(np.median(rp))
    model = 3.8 + f32_bytes[k] * ratio[k] / 7.3e6
    expect_save = (mf - 3.8) * (1 - ratio[k])
    print(f"| {k} | {mf:.2f} | {mp:.2f} | {mp / mf:.4f} | {model:.2f} | {(mf - mp) / expect_save:.2f} | {max(rp) < min(rf)} | "
          f"{' '.join(f'{x:.2f}' for x in rf)} | {' '.join(f'{x:.2f}' for x in rp)} |", flush=True)
    if tl:
        n_last = 1 if k == "cls" else min(16, cfg.n_layers)
        for name, s in (("f32", s_f), ("packed", s_p)):
            s.time_kind(k, pos, w, reps=1); s.synchronize()
            tl_rows.append((k, name, stamps(n_last)))
if tl:
    print("\nrow kernel, in-kernel stamps (us after the launch's first block entry; median block / last block):\n")
    print("| kind | form | blocks | batches per block | entry | first batch requested | x staged | first unit done | last unit done | exit | steady us per batch |\n|---|---|---:|---:|---|---|---|---|---|---|---|")
    for k, name, m in tl_rows:
        cells = [f"{m[1 + 2 * j]:.2f} / {m[2 + 2 * j]:.2f}" for j in range(7)]
        print(f"| {k} | {name} | {int(m[0])} | {m[15]:.1f} | " + " | ".join(cells) + " |")
