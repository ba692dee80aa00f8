#!/usr/bin/env python3
"""The wide step on int8 group-quantized weights (l2z_transformer_wide_q8), measured on the llama2-7b shape
at seq_len 1024 (both weight sets and 128 caches fit) with synthetic weights quantized on the device, one process:

    l2z_transformer_wide_q8 at n = 16, 32, 64, 128 rows, every row at position `pos` of its own cache, against the loop of
    l2z_transformer_batch_q8 calls of 16 over the same sequences and the f32 l2z_transformer_wide

at two depths.  Every figure is the host clock around `iters` calls back to back that end in a stream synchronise, per call;
the best of `reps` such readings after a warm-up, with the spread (max - min) / min.  Prints one JSON line a figure and, with
--md, the table of profiles/q8_wide_bench.md.

    python scripts/q8_wide_bench.py --md q8_wide_table.md
    python scripts/q8_wide_bench.py --trace-step    (for a kernel trace of its own: one wide step and one prompt pass at 32,
                                                     64 and 128 rows -- the new form and q8_gemm_kernel at the same products)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ROWS = [16, 32, 64, 128]


def best_of(fn, reps):
    fn()   # warm-up: code objects, scratch
    ts = [fn() for _ in range(reps)]
    return min(ts), (max(ts) - min(ts)) / min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--gs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--depths", type=lambda v: [int(x) for x in v.split(",")], default=[16, 500])
    ap.add_argument("--md")
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
    toks = np.random.default_rng(11).integers(2, cfg.vocab_size, 128).astype(np.int32)
    if a.trace_step:
        w32.close()
        states = [B.RunState(cfg) for _ in range(128)]
        for n in ROWS[1:]:
            for _ in range(2):   # (the second of each is the warm one)
                B.transformer_wide_q8(states[:n], toks[:n], [16] * n, w)
                states[0].prefill_q8(toks[:n], 16, w)
        return
    states = [B.RunState(cfg) for _ in range(128)]
    rows = []

    def timed(step):
        def run():
            t0 = time.perf_counter()
            for _ in range(a.iters):
                step()
            for s in states[::16]:   # (a loop's calls run on their own first runstate's stream)
                s.synchronize()
            return 1e3 * (time.perf_counter() - t0) / a.iters
        return run

    for pos in a.depths:
        for n in ROWS:
            calls = {"wide_q8": lambda: B.transformer_wide_q8(states[:n], toks[:n], [pos] * n, w, want_next=False),
                     "batch_q8 x n/16": lambda: [B.transformer_batch_q8(states[i:i + 16], toks[i:i + 16], [pos] * 16, w) for i in range(0, n, 16)],
                     "f32 wide": lambda: B.transformer_wide(states[:n], toks[:n], [pos] * n, w32, want_next=False)}
            for call, step in calls.items():
                ms, sp = best_of(timed(step), a.reps)
                r = {"call": call, "rows": n, "pos": pos, "ms": ms, "spread": sp, "reps": a.reps, "iters": a.iters,
                     "layers": a.layers, "gs": a.gs, "device": name, "cus": cus}
                rows.append(r)
                print(json.dumps(r), flush=True)
    if a.md:
        get = {(r["call"], r["rows"], r["pos"]): r for r in rows}
        cell = lambda k: f"{get[k]['ms']:.2f} ({100 * get[k]['spread']:.1f} %)"  # noqa: E731
        with open(a.md, "w") as f:
            f.write(f"{name}, {cus} CUs; llama2-7b shape with {a.layers} layers at seq_len 1024, group size {a.gs}, synthetic weights "
                    f"quantized on the device; `scripts/q8_wide_bench.py`, one process; host clock around {a.iters} calls back to back "
                    f"ending in a synchronise, per call; best of {a.reps} readings after a warm-up, spread = (max - min) / min.\n")
            for pos in a.depths:
                f.write(f"\n## position {pos}\n\n| rows | l2z_transformer_wide_q8 ms (spread) | loop of l2z_transformer_batch_q8 of 16 ms (spread) | "
                        "loop / wide | tokens/s wide | f32 l2z_transformer_wide ms (spread) | f32 / q8 |\n|---|---|---|---|---|---|---|\n")
                for n in ROWS:
                    ms, lp, f3 = (get[(c, n, pos)]["ms"] for c in ("wide_q8", "batch_q8 x n/16", "f32 wide"))
                    f.write(f"| {n} | {cell(('wide_q8', n, pos))} | {cell(('batch_q8 x n/16', n, pos))} | {lp / ms:.2f}x | {1e3 * n / ms:.0f} | "
                            f"{cell(('f32 wide', n, pos))} | {f3 / ms:.2f}x |\n")
    for r in states:
        r.close()
    w.close(); w32.close()


if __name__ == "__main__":
    main()
