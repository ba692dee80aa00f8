#!/usr/bin/env python3
"""Cost of drawing tokens on the device (l2z_sample_batch) against today's route, n x (l2z_probs_read + the host's
sampler), at vocab 32000.

  1. l2z_sample_batch for n = 1, 4, 16 rows with -t 1 -p 0.9 and -t 1 -p 1, on a near-uniform distribution (a synthetic
     model's logits: ~29k candidates at p = 0.9, the worst case) and a peaked one (the same logits x 20, placed with
     l2z_logits_write): device time per launch (l2z_sample_time, events) and wall time per call (upload, launch, copy
     back, sync).
  2. The same draws by today's route: wall time of n x (l2z_probs_read + sample / sample_top_p of libllama2_host.so).
  3. The 7B shape at n = 16 (synthetic weights, short context): tokens/s of (l2z_transformer_batch + l2z_sample_batch)
     against (l2z_transformer_batch + l2z_argmax_batch), wall clock over --window seconds each.

  python scripts/sample_bench.py [--window 1.0] [--no-7b] [--out profiles/xxx.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

NS = (1, 4, 16)


def host_lib():
    L = C.CDLL(os.path.join(ROOT, "llama2.zig_amd", "host", "libllama2_host.so"))
    fp = C.POINTER(C.c_float)
    L.l2zh_sample_coin.restype = C.c_size_t
    L.l2zh_sample_coin.argtypes = [fp, C.c_size_t, C.c_float]
    L.l2zh_sample_top_p_coin.restype = C.c_size_t
    L.l2zh_sample_top_p_coin.argtypes = [fp, C.c_size_t, C.c_float, C.c_float, fp]
    return L


def wall(fn, window):
    fn()
    t0, k = time.perf_counter(), 0
    while True:
        fn()
        k += 1
        el = time.perf_counter() - t0
        if el >= window and k >= 5:
            return el / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--no-7b", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    H = host_lib()
    res = {"device": B.device_info(0)[0], "sampler": [], "step": []}

    cfg = ck.Config(dim=288, hidden_dim=768, n_layers=2, n_heads=6, n_kv_heads=6, vocab_size=32000, seq_len=64)
    w = B.Weights(cfg, None, True, seed=15)
    ss = [B.RunState(cfg) for _ in range(max(NS))]
    ss[0].transformer(1, 0, w)
    near = ss[0].logits()
    dists = {"near-uniform": near, "peaked (x20)": near * np.float32(20.0)}
    coins = np.random.default_rng(1).uniform(0.0, 1.0, max(NS)).astype(np.float32)
    for dname, lg in dists.items():
        for s in ss:
            s.write_logits(lg)
        probs = ss[0].probs(1.0)
        n_cand = int(np.count_nonzero(probs >= np.float32(0.1) / np.float32(31999.0)))
        for top_p in (0.9, 1.0):
            for n in NS:
                st, cs = ss[:n], coins[:n]
                probe = B.sample_time(st, 1.0, top_p, cs, 3)
                iters = max(10, int(a.window * 1000.0 / max(probe, 1e-3)))
                dev_ms = B.sample_time(st, 1.0, top_p, cs, iters)
                call_ms = 1e3 * wall(lambda: B.sample_batch(st, 1.0, top_p, cs), a.window)

                def today():
                    for i in range(n):
                        pr = st[i].probs(1.0)
                        pp = pr.ctypes.data_as(C.POINTER(C.c_float))
                        if top_p == 1.0:
                            H.l2zh_sample_coin(pp, pr.size, C.c_float(cs[i]))
                        else:
                            H.l2zh_sample_top_p_coin(pp, pr.size, C.c_float(top_p), C.c_float(cs[i]), None)
                host_ms = 1e3 * wall(today, a.window)
                r = {"dist": dname, "candidates_p0.9": n_cand, "top_p": top_p, "n": n, "device_ms": round(dev_ms, 4),
                     "call_ms": round(call_ms, 4), "host_route_ms": round(host_ms, 4),
                     "speedup": round(host_ms / call_ms, 2)}
                res["sampler"].append(r)
                print(json.dumps(r), flush=True)
    for s in ss:
        s.close()
    w.close()

    if not a.no_7b:
        cfg = ck.LLAMA2_7B
        w = B.Weights(cfg, None, False, seed=2024)
        n = 16
        ss = [B.RunState(cfg) for _ in range(n)]
        toks = [7 + i for i in range(n)]
        pos = [3 + i for i in range(n)]
        cs = coins[:n]
        B.transformer_batch(ss, toks, pos, w)
        step_ms = B.batch_time(ss, toks, pos, w, 20)
        sample_dev_ms = B.sample_time(ss, 1.0, 0.9, cs, 20)

        def greedy():
            B.transformer_batch(ss, toks, pos, w)
            B.argmax_batch(ss)

        def sampled():
            B.transformer_batch(ss, toks, pos, w)
            B.sample_batch(ss, 1.0, 0.9, cs)
        g_ms = 1e3 * wall(greedy, a.window)
        s_ms = 1e3 * wall(sampled, a.window)
        r = {"shape": "llama2-7b", "n": n, "step_device_ms": round(step_ms, 4), "sample_device_ms": round(sample_dev_ms, 4),
             "sample_frac_of_step": round(sample_dev_ms / step_ms, 4),
             "greedy_ms_per_step": round(g_ms, 4), "greedy_tokens_per_s": round(n * 1e3 / g_ms, 1),
             "sampled_ms_per_step": round(s_ms, 4), "sampled_tokens_per_s": round(n * 1e3 / s_ms, 1),
             "sampled_vs_greedy": round(g_ms / s_ms, 4)}
        res["step"].append(r)
        print(json.dumps(r), flush=True)
        for s in ss:
            s.close()
        w.close()

    print("\n| distribution | top_p | n | device ms / launch | ms / call | today's route ms | x |")
    print("|---|---:|---:|---:|---:|---:|---:|")
    for r in res["sampler"]:
        print(f"| {r['dist']} | {r['top_p']} | {r['n']} | {r['device_ms']:.3f} | {r['call_ms']:.3f} | "
              f"{r['host_route_ms']:.3f} | {r['speedup']:.1f} |")
    for r in res["step"]:
        print(f"\n7B n = 16: step {r['step_device_ms']:.3f} ms, sampler {r['sample_device_ms']:.3f} ms "
              f"({100 * r['sample_frac_of_step']:.1f} % of the step); greedy {r['greedy_tokens_per_s']:.0f} tok/s, "
              f"sampled {r['sampled_tokens_per_s']:.0f} tok/s ({100 * r['sampled_vs_greedy']:.1f} %)")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
