#!/usr/bin/env python3
"""Decode from int8 group-quantized weights against the f32 decode, measured: tokens/s of
l2z_greedy_run on the full llama2-7b shape, and per kind of launch the duration (l2z_time_kind) and the effective rate of
the weight bytes it streams.  Synthetic f32 weights, quantized on the device (l2z_weights_init_q8_from).  Prints markdown:

    python scripts/q8_bench.py [--layers N] [--gs 32|64] [--steps K] > profiles/q8_bench.md
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def tokens_per_s(s, w, steps, readings=5):
    out = []
    for i in range(readings + 1):
        s.greedy_begin([])
        t0 = time.perf_counter()
        n = len(s.greedy_run(w, steps))
        dt = time.perf_counter() - t0
        if i:   # (the first reading captures the graphs)
            out.append(n / dt)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--gs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--pos", type=int, default=64)
    a = ap.parse_args()
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    c7 = ck.LLAMA2_7B
    cfg = ck.Config(c7.dim, c7.hidden_dim, a.layers, c7.n_heads, c7.n_kv_heads, c7.vocab_size, c7.seq_len)
    name, cus, _ = B.device_info(0)
    w32 = B.Weights(cfg, None, False, seed=5)
    w8 = B.Weights.quantized(w32, a.gs)
    s32, s8 = B.RunState(cfg), B.RunState(cfg)
    r32, r8 = tokens_per_s(s32, w32, a.steps), tokens_per_s(s8, w8, a.steps)
    dim, hid, kvd, V, gs = cfg.dim, cfg.hidden_dim, cfg.kv_dim, cfg.vocab_size, a.gs
    weights = {"qkv": (dim + 2 * kvd) * dim, "wo": dim * dim, "ffn13": 2 * hid * dim, "ffn2": dim * hid, "cls": V * dim}
    per_token = a.layers * sum(v for k, v in weights.items() if k != "cls") + weights["cls"]
    print(f"# int8 group-quantized decode against the f32 decode\n")
    print(f"{name}, {cus} CUs; llama2-7b shape with {a.layers} layers, group size {gs}, synthetic weights quantized on the device; "
          f"`python scripts/q8_bench.py --layers {a.layers} --gs {gs} --steps {a.steps}`.\n")
    print(f"Weight bytes a token: f32 {4 * per_token / 1e9:.2f} GB, q8 {per_token * (1 + 4 / gs) / 1e9:.2f} GB "
          f"(values + one f32 scale per {gs}): {4 / (1 + 4 / gs):.2f}x fewer.\n")
    print(f"## tokens/s, l2z_greedy_run, {a.steps} positions from BOS, median of 5 (min .. max)\n")
    print("| weights | tokens/s | ms a token |\n|---|---|---|")
    print(f"| f32 (29-bit packed stream) | {r32[0]:.1f} ({r32[1]:.1f} .. {r32[2]:.1f}) | {1e3 / r32[0]:.3f} |")
    print(f"| q8 | {r8[0]:.1f} ({r8[1]:.1f} .. {r8[2]:.1f}) | {1e3 / r8[0]:.3f} |")
    print(f"\nq8 / f32: **{r8[0] / r32[0]:.2f}x**\n")
    print(f"## per kind of launch, l2z_time_kind at position {a.pos} (us a launch; GB/s of the weight bytes: f32 at 4 bytes a weight, q8 with its scales)\n")
    print("| kind | f32 us | f32 GB/s | q8 us | q8 GB/s | f32 / q8 | q8 us a token |\n|---|---|---|---|---|---|---|")
    tot32 = tot8 = 0.0
    for kind in ("qkv", "attn", "wo", "ffn13", "ffn2", "cls", "argmax"):
        ms32, _ = s32.time_kind(kind, a.pos, w32, reps=4)
        ms8, _ = s8.time_kind(kind, a.pos, w8, reps=4)
        per = 1 if kind in ("cls", "argmax") else a.layers
        tot32 += per * ms32
        tot8 += per * ms8
        if kind in weights:
            g32 = 4 * weights[kind] / (ms32 * 1e-3) / 1e9
            g8 = weights[kind] * (1 + 4 / gs) / (ms8 * 1e-3) / 1e9
            print(f"| {kind} | {1e3 * ms32:.1f} | {g32:.0f} | {1e3 * ms8:.1f} | {g8:.0f} | {ms32 / ms8:.2f} | {1e3 * per * ms8:.0f} |")
        else:
            print(f"| {kind} | {1e3 * ms32:.1f} | - | {1e3 * ms8:.1f} | - | {ms32 / ms8:.2f} | {1e3 * per * ms8:.0f} |")
    print(f"\nSum of the kinds' durations a token: f32 {tot32:.3f} ms, q8 {tot8:.3f} ms.")
    for x in (s32, s8, w32, w8):
        x.close()


if __name__ == "__main__":
    main()
