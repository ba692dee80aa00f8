#!/usr/bin/env python3
"""Wall time of --steps decode steps of n sequences with every row's draw: ONE l2z_wide_run call against the step loop it
replaces -- per step one l2z_transformer_wide call (out_next = NULL) and ceil(n / 16) l2z_sample_batch calls -- and, for
greedy rows, against binding.generate_wide (one synchronous l2z_transformer_wide call per step).  n = 32, 64, 128 on the 7B
dims (seq_len 1024, so that 128 caches of 1 GB fit beside 27 GB of weights) and the stories110M dims, greedy and at
(temperature 1.0, top_p 0.9), at short context (every position of the run below 64) and from pos ~ 500.  Synthetic
weights; the KV rows' contents do not change the work, so no history is fed.

Each point: a warm-up of every form, then --rounds rounds in which the forms ALTERNATE in one process; a round is the
whole run of --steps steps by a host clock, ending in a synchronize of every runstate; the best round of each form is
reported as ms per step and total tokens/s.  `host ms` is the time the l2z_wide_run call itself takes on the host clock
(it is synchronous: enqueue, device time, one copy, one sync).  Prints one JSON line per point and a table; a point that
fails or is left out is listed as not run.

  python scripts/wide_run_bench.py [--shapes 7b,110m] [--ns 32,64,128] [--steps 32] [--rounds 3] [--out profiles/xxx.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="7b,110m")
    ap.add_argument("--ns", default="32,64,128")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    seven = ck.LLAMA2_7B
    shapes = {"7b": ("llama2-7b (seq_len 1024)", ck.Config(seven.dim, seven.hidden_dim, seven.n_layers, seven.n_heads,
                                                          seven.n_kv_heads, seven.vocab_size, 1024)),
              "110m": ("stories110M", ck.STORIES110M)}
    ns, steps = [int(x) for x in a.ns.split(",")], a.steps
    rows, not_run = [], []
    for key in a.shapes.split(","):
        name, cfg = shapes[key]
        w = B.Weights(cfg, None, False, seed=2024)
        ss = [B.RunState(cfg) for _ in range(max(ns))]
        for deep in (False, True):
            for n in ns:
                for sampled in (False, True):
                    point = (name, "pos ~500" if deep else "short", n, "(1.0, 0.9)" if sampled else "greedy")
                    try:
                        rows.append(measure(B, np, cfg, w, ss[:n], deep, sampled, steps, a.rounds, point))
                        print(json.dumps(rows[-1]), flush=True)
                    except Exception as e:   # the table says so
                        not_run.append((point, repr(e)))
                        print(f"NOT RUN {point}: {e!r}", flush=True)
        for s in ss:
            s.close()
        w.close()
    print("\n| shape | context | n | draw | run ms / step | loop ms / step | generate_wide ms / step | run tokens/s | loop tokens/s "
          "| loop / run | run host ms |")
    print("|---|---|---:|---|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        gw = f"{r['generate_wide_ms_per_step']:.3f}" if r["generate_wide_ms_per_step"] is not None else "--"
        print(f"| {r['shape']} | {r['context']} ({r['pos_min']}-{r['pos_max'] + steps - 1}) | {r['n']} | {r['draw']} | "
              f"{r['run_ms_per_step']:.3f} | {r['loop_ms_per_step']:.3f} | {gw} | {r['run_tokens_per_s']:.0f} | "
              f"{r['loop_tokens_per_s']:.0f} | {r['ratio']:.2f} | {r['run_host_ms']:.2f} |")
    print("\nNot run: " + ("; ".join(f"{p}: {e}" for p, e in not_run) if not_run else "none -- every cell above was measured"))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": B.device_info(0)[0], "steps": steps, "rows": rows, "not_run": not_run}, f, indent=1)


def measure(B, np, cfg, w, st, deep, sampled, steps, rounds, point):
    n = len(st)
    rng = np.random.default_rng(n)
    pos = (rng.integers(484, 516, n) if deep else rng.integers(0, 64 - steps + 1, n)).astype(np.int32)
    tok = (7 + np.arange(n)).astype(np.int32)
    temp = np.full(n, 1.0 if sampled else 0.0, np.float32)
    topp = np.full(n, 0.9, np.float32)
    coins = rng.random((steps, n), np.float32)

    def sync():
        for s in st:
            s.synchronize()

    def run():
        t0 = time.perf_counter()
        B.wide_run(st, tok, pos, w, steps, temp if sampled else None, topp, coins)
        host = (time.perf_counter() - t0) * 1e3
        sync()
        return host

    def loop():
        t = tok
        for k in range(steps):
            B.transformer_wide(st, t, pos + k, w, want_next=False)
            t = np.concatenate([B.sample_batch(st[g:g + 16], temp[g:g + 16], topp[g:g + 16], coins[k, g:g + 16])
                                for g in range(0, n, 16)])
        sync()

    def gen():
        B.generate_wide(st, tok, pos, w, steps)
        sync()

    forms = [("run", run), ("loop", loop)] + ([] if sampled else [("gen", gen)])
    for _, f in forms:   # warm-up: allocations, code objects, every form
        f()
    t = {k: [] for k, _ in forms}
    host = []
    for _ in range(rounds):
        for k, f in forms:
            t0 = time.perf_counter()
            h = f()
            t[k].append((time.perf_counter() - t0) * 1e3)
            if k == "run":
                host.append(h)
    best = {k: min(v) for k, v in t.items()}
    return {"shape": point[0], "context": "pos ~500" if deep else "short", "n": n, "draw": point[3], "steps": steps,
            "pos_min": int(pos.min()), "pos_max": int(pos.max()), "rounds": rounds,
            "run_ms_per_step": round(best["run"] / steps, 4), "loop_ms_per_step": round(best["loop"] / steps, 4),
            "generate_wide_ms_per_step": round(best["gen"] / steps, 4) if "gen" in best else None,
            "run_tokens_per_s": round(n * steps * 1000.0 / best["run"], 1),
            "loop_tokens_per_s": round(n * steps * 1000.0 / best["loop"], 1),
            "ratio": round(best["loop"] / best["run"], 3), "run_host_ms": round(min(host), 3),
            "ms_all": {k: [round(x, 2) for x in v] for k, v in t.items()}}


if __name__ == "__main__":
    main()
