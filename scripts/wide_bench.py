#!/usr/bin/env python3
"""Wall time of one decode step of n sequences: l2z_transformer_wide (one call) against the loop of ceil(n / 16)
l2z_transformer_batch calls over the same runstates, n = 16, 32, 64, 128, on the 7B dims (seq_len 1024, so that 128 caches
of 1 GB fit beside 27 GB of weights) and the stories110M dims, at short context (pos < 32) and at pos ~ 500.  Synthetic
weights; the KV rows' contents do not change the work, so no history is fed.

Each point: a warm-up of both forms, then --rounds rounds in which the two forms ALTERNATE in one process; a round is one
step by a host clock, ending in a synchronize of every runstate; the best round of each form is reported.  `enqueue ms` is
the host time until the asynchronous wide call returns (the device idle before it): at n = 128 against n = 16 it shows
what joining and releasing 112 more streams costs the host per call.  Prints one JSON line per point and a table.

  python scripts/wide_bench.py [--shapes 7b,110m] [--ns 16,32,64,128] [--rounds 6] [--out profiles/xxx.json]
  python scripts/wide_bench.py --profile-step     # three n = 64 7B steps for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def positions(n, deep, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    return rng.integers(484, 516, size=n).astype(np.int32) if deep else rng.integers(0, 32, size=n).astype(np.int32)


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="7b,110m")
    ap.add_argument("--ns", default="16,32,64,128")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-step", action="store_true")
    a = ap.parse_args()
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    seven = ck.LLAMA2_7B
    shapes = {"7b": ("llama2-7b (seq_len 1024)", ck.Config(seven.dim, seven.hidden_dim, seven.n_layers, seven.n_heads,
                                                          seven.n_kv_heads, seven.vocab_size, 1024)),
              "110m": ("stories110M", ck.STORIES110M)}
    if a.profile_step:
        cfg = shapes["7b"][1]
        w = B.Weights(cfg, None, False, seed=2024)
        ss = [B.RunState(cfg) for _ in range(64)]
        tok, pos = np.full(64, 5, np.int32), positions(64, False, 1)
        for _ in range(3):
            B.transformer_wide(ss, tok, pos, w)
        return
    ns = [int(x) for x in a.ns.split(",")]
    rows = []
    for key in a.shapes.split(","):
        name, cfg = shapes[key]
        w = B.Weights(cfg, None, False, seed=2024)
        ss = [B.RunState(cfg) for _ in range(max(ns))]
        for deep in (False, True):
            for n in ns:
                st, pos, tok = ss[:n], positions(n, deep, n), (7 + np.arange(n)).astype(np.int32)

                def sync():
                    for s in st:
                        s.synchronize()

                def wide():
                    B.transformer_wide(st, tok, pos, w, want_next=False)
                    sync()

                def loop():
                    for g in range(0, n, 16):
                        B.transformer_batch(st[g:g + 16], tok[g:g + 16], pos[g:g + 16], w)
                    sync()

                wide(), loop(), wide(), loop()   # warm-up: allocations, code objects, both forms
                t_wide, t_loop, t_enq = [], [], []
                for _ in range(a.rounds):
                    for f, out in ((wide, t_wide), (loop, t_loop)):
                        t0 = time.perf_counter()
                        f()
                        out.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    B.transformer_wide(st, tok, pos, w, want_next=False)
                    t_enq.append((time.perf_counter() - t0) * 1e3)
                    sync()
                r = {"shape": name, "n": n, "context": "pos ~500" if deep else "pos < 32", "pos_min": int(pos.min()),
                     "pos_max": int(pos.max()), "rounds": a.rounds, "wide_ms": round(min(t_wide), 3),
                     "loop_ms": round(min(t_loop), 3), "loop_calls": (n + 15) // 16,
                     "wide_tokens_per_s": round(n * 1000.0 / min(t_wide), 1),
                     "loop_tokens_per_s": round(n * 1000.0 / min(t_loop), 1),
                     "speedup": round(min(t_loop) / min(t_wide), 3), "wide_enqueue_ms": round(min(t_enq), 3),
                     "wide_ms_all": [round(x, 3) for x in t_wide], "loop_ms_all": [round(x, 3) for x in t_loop]}
                rows.append(r)
                print(json.dumps(r), flush=True)
        for s in ss:
            s.close()
        w.close()
    print("\n| shape | context | n | wide ms / step | loop ms / step (calls) | wide tokens/s | loop tokens/s | loop / wide | wide enqueue ms |")
    print("|---|---|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print(f"| {r['shape']} | {r['context']} ({r['pos_min']}-{r['pos_max']}) | {r['n']} | {r['wide_ms']:.3f} | "
              f"{r['loop_ms']:.3f} ({r['loop_calls']}) | {r['wide_tokens_per_s']:.0f} | {r['loop_tokens_per_s']:.0f} | "
              f"{r['speedup']:.2f} | {r['wide_enqueue_ms']:.3f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": B.device_info(0)[0], "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
