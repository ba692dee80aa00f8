"""l2z_sample_run against the two per-token routes it replaces, on the stories15M, stories110M and Llama-2-7B shapes
(synthetic weights): tokens/s of 256 generated tokens from BOS, no prompt.

Routes, all through the Python binding, wall clock, best of --rounds after a warm-up, the routes alternating:
  loop      greedy_begin + ONE RunState.sample_run call (one graph replay per position, one copy back per 64 positions)
  batch     per token l2z_transformer + l2z_sample_batch (upload, launch, copy back, sync)
  host      per token l2z_transformer + l2z_probs_read (128 KB copy, sync) + the host sampler (libllama2_host.so)
Temperatures 1.0 (near-uniform on synthetic weights: the sequential walk is long) and 0.05 (peaked), each with top_p 0.9 and 1.
The three routes draw the same ids (asserted); a run that a drawn BOS ends early is timed over the tokens it produced.

    python scripts/sample_run_bench.py [--shapes stories15M,stories110M,llama2-7b] [--out profiles/sample_run_bench.md]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_TOKENS = 256
CASES = ((1.0, 0.9), (1.0, 1.0), (0.05, 0.9), (0.05, 1.0))


def load():
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    return np, pkg.binding, pkg.checkpoint


def host_sampler():
    H = C.CDLL(os.path.join(ROOT, "llama2.zig_amd", "host", "libllama2_host.so"))
    fp = C.POINTER(C.c_float)
    H.l2zh_sample_coin.restype = C.c_size_t
    H.l2zh_sample_coin.argtypes = [fp, C.c_size_t, C.c_float]
    H.l2zh_sample_top_p_coin.restype = C.c_size_t
    H.l2zh_sample_top_p_coin.argtypes = [fp, C.c_size_t, C.c_float, C.c_float, fp]

    def draw(probs, top_p, coin):
        pp = probs.ctypes.data_as(fp)
        if top_p in (0.0, 1.0):
            return int(H.l2zh_sample_coin(pp, probs.size, C.c_float(coin)))
        return int(H.l2zh_sample_top_p_coin(pp, probs.size, C.c_float(top_p), C.c_float(coin), None))
    return draw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_run_bench.md"))
    ap.add_argument("--shapes", default="stories15M,stories110M,llama2-7b")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    np, B, ck = load()
    draw = host_sampler()
    shapes = {"stories15M": ck.STORIES15M, "stories110M": ck.STORIES110M, "llama2-7b": ck.LLAMA2_7B}
    out = [f"# l2z_sample_run, synthetic weights (scripts/sample_run_bench.py)\n\nDevice: {B.device_info(0)[0]}.  Tokens/s of "
           f"{N_TOKENS} generated tokens from BOS through the Python binding, wall clock, best of {a.rounds} after a warm-up, the "
           "routes alternating.  loop: one l2z_sample_run call; batch: l2z_transformer + l2z_sample_batch per token; host: "
           "l2z_transformer + l2z_probs_read + the host sampler per token.  The three routes draw the same ids.\n\n"
           "| shape | t | top_p | tokens | loop tok/s | batch tok/s | host tok/s | loop / batch | loop / host |\n"
           "|---|---:|---:|---:|---:|---:|---:|---:|---:|\n"]
    for name in a.shapes.split(","):
        cfg = shapes[name]
        w = B.Weights(cfg, None, name != "llama2-7b", seed=1)
        s = B.RunState(cfg)
        n = min(N_TOKENS, cfg.seq_len)
        coins = B.coin_stream(1, n)
        for t, p in CASES:
            def loop():
                return B.generate_sample(s, w, (), n, t, p, coins)

            def stepped(pick):
                token, ids = 1, []
                for pos in range(n):
                    s.transformer(token, pos, w)
                    token = pick(pos)
                    ids.append(token)
                    if token == 1:
                        break
                return np.array(ids, np.int32)
            routes = {"loop": loop,
                      "batch": lambda: stepped(lambda pos: int(B.sample_batch([s], t, p, coins[pos])[0])),
                      "host": lambda: stepped(lambda pos: draw(s.probs(t), p, float(coins[pos])))}
            ids = {k: f() for k, f in routes.items()}   # warm-up; the routes agree
            assert all(np.array_equal(ids["loop"], v) for v in ids.values()), (name, t, p)
            best = {k: float("inf") for k in routes}
            for _ in range(a.rounds):
                for k, f in routes.items():
                    t0 = time.perf_counter()
                    f()
                    best[k] = min(best[k], time.perf_counter() - t0)
            m = len(ids["loop"])
            tps = {k: m / v for k, v in best.items()}
            out.append(f"| {name} | {t} | {p} | {m} | {tps['loop']:.0f} | {tps['batch']:.0f} | {tps['host']:.0f} | "
                       f"{tps['loop'] / tps['batch']:.3f} | {tps['loop'] / tps['host']:.3f} |\n")
            print(out[-1], end="", flush=True)
        s.close()
        w.close()
    with open(a.out, "w") as f:
        f.write("".join(out))


if __name__ == "__main__":
    main()
