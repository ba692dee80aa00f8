#!/usr/bin/env python3
"""The batched prompt pass on int8 group-quantized weights (l2z_prefill_q8), measured on the llama2-7b shape
with synthetic weights quantized on the device (l2z_weights_init_q8_from): a prompt of n tokens at position 0 by

    q8       one l2z_prefill_q8 call                       (this pass)
    stepped  n l2z_transformer calls on the same q8 weights (the only way before it)
    f32      one l2z_prefill call on the f32 weights        (the bf16-core prompt pass)

A leg is one process -- run each under its own time limit -- and writes one JSON line per length: best of `reps` wall-clock
readings after a warm-up (every call ends in a stream synchronise), and the spread (max - min) / min.  --report merges the
legs' files into the markdown table of profiles/q8_prefill_bench.md:

    python scripts/q8_prefill_bench.py --leg q8 > q8.jsonl          (likewise stepped, f32)
    python scripts/q8_prefill_bench.py --report q8.jsonl stepped.jsonl f32.jsonl > profiles/q8_prefill_bench.md
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

LENGTHS = [4, 16, 32, 64, 128, 512, 1024]


def measure(fn, reps):
    fn()   # warm-up: code objects, scratch, graphs
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * min(ts), (max(ts) - min(ts)) / min(ts)


def run_leg(a):
    import numpy as np
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    c7 = ck.LLAMA2_7B
    cfg = ck.Config(c7.dim, c7.hidden_dim, a.layers, c7.n_heads, c7.n_kv_heads, c7.vocab_size, c7.seq_len)
    name, cus, _ = B.device_info(0)
    w = B.Weights(cfg, None, False, seed=5)
    if a.leg != "f32":
        w32, w = w, B.Weights.quantized(w, a.gs)
        w32.close()
    s = B.RunState(cfg)
    rng = np.random.default_rng(11)
    for n in a.lengths:
        toks = rng.integers(2, cfg.vocab_size, n).astype(np.int32)
        if a.leg == "q8":
            call = lambda: s.prefill_q8(toks, 0, w)  # noqa: E731
        elif a.leg == "f32":
            call = lambda: s.prefill(toks, 0, w)  # noqa: E731
        else:
            def call():
                for p in range(n):
                    s.transformer(int(toks[p]), p, w)
                s.synchronize()
        ms, spread = measure(call, a.reps)
        print(json.dumps({"leg": a.leg, "n": n, "ms": ms, "spread": spread, "reps": a.reps, "layers": a.layers, "gs": a.gs,
                          "device": name, "cus": cus}), flush=True)
    s.close(); w.close()


def report(paths):
    rows = {}
    meta = None
    for p in paths:
        for line in open(p):
            if line.startswith("{"):
                r = json.loads(line)
                rows.setdefault(r["n"], {})[r["leg"]] = r
                meta = r
    print("# l2z_prefill_q8 against the stepped q8 prompt and the f32 prompt pass\n")
    print(f"{meta['device']}, {meta['cus']} CUs; llama2-7b shape with {meta['layers']} layers, group size {meta['gs']}, synthetic weights "
          f"quantized on the device; `scripts/q8_prefill_bench.py`, a leg a process, best of {meta['reps']} wall-clock readings after a "
          "warm-up, spread = (max - min) / min of the readings.\n")
    print("| prompt tokens | q8 pass ms (spread) | stepped q8 ms (spread) | stepped / pass | f32 l2z_prefill ms (spread) | f32 / pass |")
    print("|---|---|---|---|---|---|")
    for n in sorted(rows):
        r = rows[n]
        cell = lambda leg: f"{r[leg]['ms']:.2f} ({100 * r[leg]['spread']:.1f} %)" if leg in r else "not measured"  # noqa: E731
        ratio = lambda leg: f"{r[leg]['ms'] / r['q8']['ms']:.2f}x" if leg in r and "q8" in r else "-"  # noqa: E731
        print(f"| {n} | {cell('q8')} | {cell('stepped')} | {ratio('stepped')} | {cell('f32')} | {ratio('f32')} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["q8", "stepped", "f32"])
    ap.add_argument("--report", nargs="+")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--gs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--lengths", type=lambda v: [int(x) for x in v.split(",")], default=LENGTHS)
    a = ap.parse_args()
    if a.report:
        report(a.report)
    elif a.leg:
        run_leg(a)
    else:
        ap.error("--leg or --report")


if __name__ == "__main__":
    main()
