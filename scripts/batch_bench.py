#!/usr/bin/env python3
"""Aggregate decode rate of the batched step (l2z_transformer_batch) for n = 1, 2, 4, 8, 16 sequences on the 7B shape
and the stories110M shape, at short context (pos < 32) and at long context (pos ~ 2000; stories110M's seq_len is 1024,
so ~1000 there).  Synthetic weights; the KV rows' contents do not change the work, so no history is fed.

Each point: a warm-up, then steps back to back timed by device events on the pass's stream (l2z_batch_time) over a
window of at least --window seconds.  Prints one JSON line per point and a table.

  python scripts/batch_bench.py [--shapes 7b,110m] [--window 1.0] [--out profiles/xxx.json]
  python scripts/batch_bench.py --profile-step     # a few n = 16 7B steps for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

NS = (1, 2, 4, 8, 16)


def positions(n, long, seq_len, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    if long:
        hi = min(2000, seq_len - 16)
        return [int(p) for p in rng.integers(hi - 16, hi + 16, size=n)]
    return [int(p) for p in rng.integers(0, 32, size=n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="7b,110m")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-step", action="store_true")
    a = ap.parse_args()
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    shapes = {"7b": ("llama2-7b", ck.LLAMA2_7B), "110m": ("stories110M", ck.STORIES110M)}
    if a.profile_step:
        cfg = ck.LLAMA2_7B
        w = B.Weights(cfg, None, False, seed=2024)
        ss = [B.RunState(cfg) for _ in range(16)]
        toks, pos = [5] * 16, positions(16, False, cfg.seq_len, 1)
        for _ in range(3):
            B.transformer_batch(ss, toks, pos, w)
        ss[0].synchronize()
        return
    rows = []
    for key in a.shapes.split(","):
        name, cfg = shapes[key]
        w = B.Weights(cfg, None, False, seed=2024)
        ss = [B.RunState(cfg) for _ in range(max(NS))]
        for long in (False, True):
            for n in NS:
                pos = positions(n, long, cfg.seq_len, n)
                toks = [7 + i for i in range(n)]
                st = ss[:n]
                probe = B.batch_time(st, toks, pos, w, 3)  # warm-up, and the step's rough cost
                iters = max(5, int(a.window * 1000.0 / max(probe, 1e-3)) + 1)
                ms = B.batch_time(st, toks, pos, w, iters)
                r = {"shape": name, "n": n, "context": "long" if long else "short", "pos_min": min(pos),
                     "pos_max": max(pos), "iters": iters, "window_s": round(ms * iters / 1000.0, 3),
                     "ms_per_step": round(ms, 4), "tokens_per_s": round(n * 1000.0 / ms, 1)}
                rows.append(r)
                print(json.dumps(r), flush=True)
        for s in ss:
            s.close()
        w.close()
    print("\n| shape | context | n | ms / step | tokens/s | x n=1 |")
    print("|---|---|---:|---:|---:|---:|")
    for r in rows:
        base = next(b for b in rows if b["shape"] == r["shape"] and b["context"] == r["context"] and b["n"] == 1)
        print(f"| {r['shape']} | {r['context']} (pos {r['pos_min']}-{r['pos_max']}) | {r['n']} | {r['ms_per_step']:.3f} | "
              f"{r['tokens_per_s']:.0f} | {r['tokens_per_s'] / base['tokens_per_s']:.2f} |")
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": B.device_info(0)[0], "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
