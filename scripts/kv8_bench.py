#!/usr/bin/env python3
"""The wide q8 step on int8 KV rows against the same step on f32 rows (l2z_transformer_wide_q8 on l2z_runstate_init_kv8
runstates), measured on the llama2-7b shape at seq_len 1024 and group size 64 with synthetic weights
quantized on the device, one process, the two kinds interleaved reading by reading:

    32 / 64 / 128 sequences, every one at position 16, 500 or 1000 of its own cache.

Every figure is the host clock around `iters` calls back to back that end in a stream synchronise, per call; the best of
`reps` such readings after a warm-up, with the spread (max - min) / min.  Prints one JSON line a figure and, with --md, the
table of profiles/kv8_bench.md.

    python scripts/kv8_bench.py --md kv8_table.md
    python scripts/kv8_bench.py --f32-only          (the f32-row figures alone: with L2Z_LIB naming an older build, what
                                                     that build gives for the same calls)
    python scripts/kv8_bench.py --trace-step        (for a kernel trace of its own: two steps of either kind at 128 rows,
                                                     position 500 -- the second of each is the warm one)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ROWS = [32, 64, 128]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--gs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--depths", type=lambda v: [int(x) for x in v.split(",")], default=[16, 500, 1000])
    ap.add_argument("--md")
    ap.add_argument("--f32-only", action="store_true")
    ap.add_argument("--trace-step", action="store_true")
    a = ap.parse_args()
    import numpy as np
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    c7 = ck.LLAMA2_7B
    cfg = ck.Config(c7.dim, c7.hidden_dim, a.layers, c7.n_heads, c7.n_kv_heads, c7.vocab_size, 1024)
    name, cus, _ = B.device_info(0)
    w32 = B.Weights(cfg, None, False, seed=5)
    w = B.Weights.quantized(w32, a.gs)
    w32.close()
    toks = np.random.default_rng(11).integers(2, cfg.vocab_size, 128).astype(np.int32)
    kinds = {"f32 rows": [B.RunState(cfg) for _ in range(128)]}
    if not a.f32_only:
        kinds["int8 rows"] = [B.RunState(cfg, kv8=True) for _ in range(128)]
    hs, per_pos = cfg.dim // cfg.n_heads, cfg.n_layers * cfg.n_kv_heads * cfg.seq_len
    cache_bytes = {"f32 rows": 2 * per_pos * hs * 4, "int8 rows": 2 * per_pos * (hs + 4)}
    if a.trace_step:
        for states in kinds.values():
            for _ in range(2):
                B.transformer_wide_q8(states, toks, [500] * 128, w)
        return

    def reading(states, n, pos):
        t0 = time.perf_counter()
        for _ in range(a.iters):
            B.transformer_wide_q8(states[:n], toks[:n], [pos] * n, w, want_next=False)
        states[0].synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.iters

    rows = []
    for pos in a.depths:
        for n in ROWS:
            ts = {k: [] for k in kinds}
            for rep in range(a.reps + 1):   # (the first reading of each kind is the warm-up)
                for k, states in kinds.items():
                    t = reading(states, n, pos)
                    if rep:
                        ts[k].append(t)
            for k, t in ts.items():
                r = {"rows_kind": k, "rows": n, "pos": pos, "ms": min(t), "spread": (max(t) - min(t)) / min(t), "reps": a.reps,
                     "iters": a.iters, "layers": a.layers, "gs": a.gs, "cache_bytes_a_sequence": cache_bytes[k], "device": name,
                     "cus": cus, "lib": os.path.basename(os.path.dirname(B.LIB_PATH)) + "/" + os.path.basename(B.LIB_PATH)}
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.md:
        get = {(r["rows_kind"], r["rows"], r["pos"]): r for r in rows}
        cell = lambda k: f"{get[k]['ms']:.2f} ({100 * get[k]['spread']:.1f} %)"  # noqa: E731
        with open(a.md, "w") as f:
            f.write(f"{name}, {cus} CUs; llama2-7b shape with {a.layers} layers at seq_len 1024, group size {a.gs}, synthetic weights "
                    f"quantized on the device; `scripts/kv8_bench.py`, one process, the kinds interleaved reading by reading; host clock "
                    f"around {a.iters} calls back to back ending in a synchronise, per call; best of {a.reps} readings after a warm-up, "
                    f"spread = (max - min) / min.  Cache bytes a sequence: " +
                    ", ".join(f"{k} {cache_bytes[k] / 2 ** 30:.3f} GiB" for k in kinds) + ".\n\n")
            f.write("| position | sequences | " + " | ".join(f"{k} ms (spread)" for k in kinds) + " | f32 / int8 |\n|---|---|" + "---|" * (len(kinds) + 1) + "\n")
            for pos in a.depths:
                for n in ROWS:
                    ratio = f"{get[('f32 rows', n, pos)]['ms'] / get[('int8 rows', n, pos)]['ms']:.2f}x" if "int8 rows" in kinds else "-"
                    f.write(f"| {pos} | {n} | " + " | ".join(cell((k, n, pos)) for k in kinds) + f" | {ratio} |\n")
    for states in kinds.values():
        for r in states:
            r.close()
    w.close()


if __name__ == "__main__":
    main()
