#!/usr/bin/env python3
"""The batched step and the verify pass on int8 group-quantized weights (l2z_transformer_batch_q8, l2z_verify_q8; DESIGN.md
4.25), measured on the llama2-7b shape with synthetic weights quantized on the device (Weights.quantized), one process:

    batch   l2z_transformer_batch_q8 at n = 1, 2, 4, 8, 16 rows, every row at position `pos` of its own cache
            against n single q8 steps (l2z_transformer) and the f32 l2z_transformer_batch
    verify  l2z_verify_q8 at 4, 8, 16 rows from position `pos` on
            against one q8 step, the f32 l2z_verify and l2z_prefill_q8 of as many tokens

at two depths.  The batched calls are timed by device events over `iters` passes back to back (l2z_batch_q8_time,
l2z_verify_q8_time and their f32 twins), the single steps and the prompt pass by the host clock around calls that end in a
stream synchronise; each figure is the best of `reps` such readings after a warm-up, with the spread (max - min) / min.
Prints one JSON line a figure and, with --md, the tables of profiles/q8_batch_bench.md.

    python scripts/q8_batch_bench.py --md q8_batch_table.md
    python scripts/q8_batch_bench.py --trace-step        (one 16-row step of each call, for a kernel trace of its own)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

BATCH_ROWS = [1, 2, 4, 8, 16]
VERIFY_ROWS = [4, 8, 16]


def best_of(fn, reps):
    fn()   # warm-up: code objects, scratch, graphs
    ts = [fn() for _ in range(reps)]
    return min(ts), (max(ts) - min(ts)) / min(ts)


def wall_ms(fn, sync):
    def timed():
        t0 = time.perf_counter()
        fn()
        sync()
        return 1e3 * (time.perf_counter() - t0)
    return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--gs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--depths", type=lambda v: [int(x) for x in v.split(",")], default=[16, 2000])
    ap.add_argument("--md")
    ap.add_argument("--trace-step", action="store_true")
    a = ap.parse_args()
    import numpy as np
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    c7 = ck.LLAMA2_7B
    cfg = ck.Config(c7.dim, c7.hidden_dim, a.layers, c7.n_heads, c7.n_kv_heads, c7.vocab_size, c7.seq_len)
    name, cus, _ = B.device_info(0)
    w32 = B.Weights(cfg, None, False, seed=5)
    w = B.Weights.quantized(w32, a.gs)
    states = [B.RunState(cfg) for _ in range(16)]
    s = states[0]
    rng = np.random.default_rng(11)
    toks = rng.integers(2, cfg.vocab_size, 16).astype(np.int32)
    if a.trace_step:
        pos = min(a.depths[-1], cfg.seq_len - 16)
        for _ in range(2):   # (the second of each is the warm one)
            B.transformer_batch_q8(states, toks, [pos] * 16, w)
            s.verify_q8(toks, pos, w)
        s.synchronize()
        return
    rows = []

    def put(call, n, pos, ms, spread, how):
        r = {"call": call, "rows": n, "pos": pos, "ms": ms, "spread": spread, "how": how, "reps": a.reps, "iters": a.iters,
             "layers": a.layers, "gs": a.gs, "device": name, "cus": cus}
        rows.append(r)
        print(json.dumps(r), flush=True)

    for pos in a.depths:
        pos = min(pos, cfg.seq_len - 16)
        ms, sp = best_of(wall_ms(lambda: [s.transformer(int(toks[0]), pos, w) for _ in range(a.iters)], s.synchronize), a.reps)
        put("q8 step", 1, pos, ms / a.iters, sp, "host clock")
        for n in BATCH_ROWS:
            ms, sp = best_of(lambda: B.batch_q8_time(states[:n], toks[:n], [pos] * n, w, a.iters), a.reps)
            put("batch_q8", n, pos, ms, sp, "device events")
        ms, sp = best_of(lambda: B.batch_time(states, toks, [pos] * 16, w32, a.iters), a.reps)
        put("f32 batch", 16, pos, ms, sp, "device events")
        for n in VERIFY_ROWS:
            ms, sp = best_of(lambda: s.verify_q8_time(toks[:n], pos, w, a.iters), a.reps)
            put("verify_q8", n, pos, ms, sp, "device events")
            ms, sp = best_of(lambda: s.verify_time(toks[:n], pos, w32, a.iters), a.reps)
            put("f32 verify", n, pos, ms, sp, "device events")
            ms, sp = best_of(wall_ms(lambda: s.prefill_q8(toks[:n], pos, w), lambda: None), a.reps)
            put("prefill_q8", n, pos, ms, sp, "host clock")
    if a.md:
        get = {(r["call"], r["rows"], r["pos"]): r for r in rows}
        cell = lambda k: f"{get[k]['ms']:.2f} ({100 * get[k]['spread']:.1f} %)" if k in get else "not measured"  # noqa: E731
        with open(a.md, "w") as f:
            f.write(f"{name}, {cus} CUs; llama2-7b shape with {a.layers} layers, group size {a.gs}, synthetic weights quantized on "
                    f"the device; `scripts/q8_batch_bench.py`, one process; best of {a.reps} readings after a warm-up, spread = "
                    f"(max - min) / min; batched calls: device events over {a.iters} passes back to back; single steps and the "
                    "prompt pass: host clock around calls that end in a synchronise.\n")
            for pos in sorted({r["pos"] for r in rows}):
                step = get[("q8 step", 1, pos)]["ms"]
                f.write(f"\n## position {pos}\n\none q8 step (l2z_transformer): {cell(('q8 step', 1, pos))} ms\n\n")
                f.write("| rows | l2z_transformer_batch_q8 ms (spread) | n single q8 steps ms | single / batched | tokens/s batched | f32 l2z_transformer_batch ms |\n|---|---|---|---|---|---|\n")
                for n in BATCH_ROWS:
                    ms = get[("batch_q8", n, pos)]["ms"]
                    f.write(f"| {n} | {cell(('batch_q8', n, pos))} | {n * step:.2f} | {n * step / ms:.2f}x | {1e3 * n / ms:.0f} | "
                            f"{cell(('f32 batch', n, pos))} |\n")
                f.write("\n| rows | l2z_verify_q8 ms (spread) | in q8 steps | f32 l2z_verify ms (spread) | l2z_prefill_q8 ms (spread) |\n|---|---|---|---|---|\n")
                for n in VERIFY_ROWS:
                    ms = get[("verify_q8", n, pos)]["ms"]
                    f.write(f"| {n} | {cell(('verify_q8', n, pos))} | {ms / step:.2f} | {cell(('f32 verify', n, pos))} | "
                            f"{cell(('prefill_q8', n, pos))} |\n")
    for r in states:
        r.close()
    w.close(); w32.close()


if __name__ == "__main__":
    main()
