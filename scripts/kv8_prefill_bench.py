#!/usr/bin/env python3
"""A prompt into int8 KV rows: l2z_prefill_kv8 against the route it replaces -- l2z_prefill_q8 on an f32 runstate, then
l2z_runstate_fork into a kv8 one --, measured on the llama2-7b shape at group size 64 with synthetic
weights quantized on the device, one process, the two routes interleaved reading by reading:

    128, 512 and 1024 tokens at position 0 of seq_len 1024; 512 tokens at position 1024 of seq_len 2048.

Every figure is the host clock around one route (both calls are synchronous), the best of `reps` readings after a warm-up,
with the spread (max - min) / min.  Device memory at peak is each route's WHOLE footprint, weights apart, by hipMemGetInfo's
used bytes: the direct route's kv8 runstate and its scratch; the fork route's f32 runstate, its scratch AND the kv8
runstate it fills.  Prints one JSON line a figure and, with --md, the table of profiles/kv8_prefill_bench.md.

    python scripts/kv8_prefill_bench.py --md kv8_prefill_table.md
    python scripts/kv8_prefill_bench.py --trace      (for a kernel trace of its own: seq_len 2048 alone, each route twice on
                                                      512 tokens at position 1024 and nothing else, so every attention
                                                      launch of the trace is that chunk's; the rows below it are not
                                                      written: a kernel's time does not depend on what they hold)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

CASES = [(1024, 0, 128), (1024, 0, 512), (1024, 0, 1024), (2048, 1024, 512)]   # (seq_len, pos0, tokens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--gs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--md")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    c7 = ck.LLAMA2_7B
    name, cus, _ = B.device_info(0)
    used = lambda: (lambda free, total: total - free)(*torch.cuda.mem_get_info(0))  # noqa: E731
    rows = []
    for seq_len in ([2048] if a.trace else sorted({c[0] for c in CASES})):
        cfg = ck.Config(c7.dim, c7.hidden_dim, a.layers, c7.n_heads, c7.n_kv_heads, c7.vocab_size, seq_len)
        w32 = B.Weights(cfg, None, False, seed=5)
        w = B.Weights.quantized(w32, a.gs)
        w32.close()
        toks = np.random.default_rng(11).integers(2, cfg.vocab_size, seq_len).astype(np.int32)
        base = used()
        s8 = B.RunState(cfg, kv8=True)

        def direct(pos0, n):
            s8.prefill_kv8(toks[pos0:pos0 + n], pos0, w)

        if not a.trace:
            direct(0, 1024)   # (rows 0 .. 1023 stand for the deep case; the scratch at its largest)
        peak = {"prefill_kv8": used() - base}
        base_fork = used()
        f32, dst = B.RunState(cfg), B.RunState(cfg, kv8=True)

        def forked(pos0, n):
            f32.prefill_q8(toks[pos0:pos0 + n], pos0, w)
            B.runstate_fork(dst, f32, pos0 + n)
            dst.synchronize()

        if not a.trace:
            forked(0, 1024)
        peak["prefill_q8 + fork"] = used() - base_fork   # (the f32 runstate, its scratch and the kv8 runstate it fills)
        routes = {"prefill_kv8": direct, "prefill_q8 + fork": forked}
        for S, pos0, n in CASES:
            if S != seq_len:
                continue
            if a.trace:
                if pos0:
                    for fn in routes.values():
                        fn(pos0, n), fn(pos0, n)
                continue
            ts = {k: [] for k in routes}
            for rep in range(a.reps + 1):   # (the first reading of each route is the warm-up)
                for k, fn in routes.items():
                    t0 = time.perf_counter()
                    fn(pos0, n)
                    if rep:
                        ts[k].append(1e3 * (time.perf_counter() - t0))
            for k, t in ts.items():
                r = {"route": k, "seq_len": S, "pos0": pos0, "tokens": n, "ms": min(t), "spread": (max(t) - min(t)) / min(t),
                     "reps": a.reps, "layers": a.layers, "gs": a.gs, "peak_bytes": peak[k], "device": name, "cus": cus}
                rows.append(r)
                print(json.dumps(r), flush=True)
        for r in (s8, f32, dst, w):
            r.close()
    if a.md and rows:
        get = {(r["route"], r["seq_len"], r["pos0"], r["tokens"]): r for r in rows}
        cell = lambda k: f"{get[k]['ms']:.2f} ({100 * get[k]['spread']:.1f} %)"  # noqa: E731
        with open(a.md, "w") as f:
            f.write(f"{name}, {cus} CUs; llama2-7b shape with {a.layers} layers, group size {a.gs}, synthetic weights quantized on the "
                    f"device; `scripts/kv8_prefill_bench.py`, one process, the routes interleaved reading by reading; host clock around "
                    f"one route, best of {a.reps} readings after a warm-up, spread = (max - min) / min; peak = the route's WHOLE device "
                    f"footprint, weights apart: the kv8 runstate and its scratch, against the f32 runstate, its scratch and the kv8 "
                    f"runstate it fills.\n\n")
            f.write("| seq_len | pos0 | tokens | prefill_kv8 ms (spread) | prefill_q8 + fork ms (spread) | fork route / kv8 | peak GiB kv8 | peak GiB fork route |\n"
                    "|---|---|---|---|---|---|---|---|\n")
            for S, pos0, n in CASES:
                d, k = get[("prefill_kv8", S, pos0, n)], get[("prefill_q8 + fork", S, pos0, n)]
                f.write(f"| {S} | {pos0} | {n} | {cell(('prefill_kv8', S, pos0, n))} | {cell(('prefill_q8 + fork', S, pos0, n))} | "
                        f"{k['ms'] / d['ms']:.2f}x | {d['peak_bytes'] / 2 ** 30:.3f} | {k['peak_bytes'] / 2 ** 30:.3f} |\n")


if __name__ == "__main__":
    main()
