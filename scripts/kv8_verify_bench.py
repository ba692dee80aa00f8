#!/usr/bin/env python3
"""Guessed rows over int8 KV rows: l2z_verify_kv8 against what the same rows cost without it -- l2z_prefill_kv8 of those rows
at that position, whose row form sends every row through kv8_attention as a one-row sequence --, measured
on the llama2-7b shape at group size 64 with synthetic weights quantized on the device, one process, one kv8 runstate of
seq_len 2048 that holds 2016 prompt rows:

    4, 8 and 16 rows at positions 16, 500 and 2000; and one l2z_transformer_wide_q8 step (n = 1) at each position.

verify_kv8: l2z_verify_kv8_time (device events over `iters` passes back to back, verdict and copy included).  prefill_kv8 and
the step: the host clock around `iters` calls between two device synchronizes (both calls are synchronous; the prompt call
ends in the decode's classifier launch on one row, the verify pass in one product over all rows and the verdict).  The three
are interleaved reading by reading; a figure is the best of `reps` readings after a warm-up, with the spread
(max - min) / min.  "depth" is a route's time at position 2000 less its time at position 16 with the same rows: the part
of the pass that grows with the rows read, which is the attention's.  Prints one JSON line a figure and, with --md, the
table of profiles/kv8_verify_bench.md.

    python scripts/kv8_verify_bench.py --md kv8_verify_table.md
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

SEQ_LEN, POSITIONS, ROWS = 2048, (16, 500, 2000), (4, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--gs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--md")
    a = ap.parse_args()
    import numpy as np
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    c7 = ck.LLAMA2_7B
    name, cus, _ = B.device_info(0)
    cfg = ck.Config(c7.dim, c7.hidden_dim, a.layers, c7.n_heads, c7.n_kv_heads, c7.vocab_size, SEQ_LEN)
    w32 = B.Weights(cfg, None, False, seed=5)
    w = B.Weights.quantized(w32, a.gs)
    w32.close()
    toks = np.random.default_rng(11).integers(2, cfg.vocab_size, SEQ_LEN).astype(np.int32)
    s = B.RunState(cfg, kv8=True)
    s.prefill_kv8(toks[:max(POSITIONS) + max(ROWS)], 0, w)   # every row a case reads stands; every case rewrites its own

    def hosted(call):   # ms a call, the host clock between two device synchronizes
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            call()
        s.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.iters

    got = {}
    for pos in POSITIONS:
        for n in ROWS:
            t = toks[pos:pos + n]
            routes = {"verify_kv8": lambda: s.verify_kv8_time(t, pos, w, a.iters),
                      "prefill_kv8": lambda: hosted(lambda: s.prefill_kv8(t, pos, w))}
            if n == ROWS[0]:
                routes["wide_q8 step"] = lambda: hosted(lambda: B.transformer_wide_q8([s], [int(t[0])], [pos], w, want_next=False))
            ts = {k: [] for k in routes}
            for rep in range(a.reps + 1):   # (the first reading of each route is the warm-up)
                for k, fn in routes.items():
                    ms = fn()
                    if rep:
                        ts[k].append(ms)
            for k, v in ts.items():
                r = {"route": k, "pos0": pos, "rows": 1 if k == "wide_q8 step" else n, "ms": min(v), "spread": (max(v) - min(v)) / min(v),
                     "reps": a.reps, "iters": a.iters, "layers": a.layers, "gs": a.gs, "seq_len": SEQ_LEN, "device": name, "cus": cus}
                got[(k, pos, r["rows"])] = r
                print(json.dumps(r), flush=True)
    for r in (s, w):
        r.close()
    if a.md:
        cell = lambda k: f"{got[k]['ms']:.3f} ({100 * got[k]['spread']:.1f} %)"  # noqa: E731
        depth = lambda k, n: got[(k, POSITIONS[-1], n)]["ms"] - got[(k, POSITIONS[0], n)]["ms"]  # noqa: E731
        with open(a.md, "w") as f:
            f.write(f"{name}, {cus} CUs; llama2-7b shape with {a.layers} layers, seq_len {SEQ_LEN}, group size {a.gs}, synthetic weights "
                    f"quantized on the device; `scripts/kv8_verify_bench.py`, one process, the routes interleaved reading by reading; "
                    f"verify_kv8 by device events over {a.iters} passes, the other two by the host clock around {a.iters} synchronous "
                    f"calls; best of {a.reps} readings after a warm-up, spread = (max - min) / min.\n\n")
            f.write("| pos0 | rows | verify_kv8 ms (spread) | prefill_kv8 ms (spread) | prefill / verify | wide_q8 step (1 row) ms |\n|---|---|---|---|---|---|\n")
            for pos in POSITIONS:
                for n in ROWS:
                    f.write(f"| {pos} | {n} | {cell(('verify_kv8', pos, n))} | {cell(('prefill_kv8', pos, n))} | "
                            f"{got[('prefill_kv8', pos, n)]['ms'] / got[('verify_kv8', pos, n)]['ms']:.2f}x | "
                            f"{cell(('wide_q8 step', pos, 1)) if n == ROWS[0] else ''} |\n")
            f.write(f"\nDepth cost, position {POSITIONS[-1]} less position {POSITIONS[0]} at the same rows (the attention's part):\n\n"
                    "| rows | verify_kv8 ms | prefill_kv8 (row form) ms | verify / row form | 1 / rows |\n|---|---|---|---|---|\n")
            for n in ROWS:
                f.write(f"| {n} | {depth('verify_kv8', n):.3f} | {depth('prefill_kv8', n):.3f} | "
                        f"{depth('verify_kv8', n) / depth('prefill_kv8', n):.3f} | {1 / n:.3f} |\n")


if __name__ == "__main__":
    main()
