"""l2z_score against l2z_prefill on the 7B shape: what scoring every position costs on top of ingesting them.

One process holds this build; with --parent-lib a CHILD process holds another build of the library (the parent commit's
libllama2_hip_test.so, loaded the way L2Z_LIB points the binding at another build) and times its l2z_prefill on request,
so that the two builds alternate inside one run on one GPU.  Per length (128 / 512 / 1024 tokens), after a warm-up of
every leg, 6 rounds of: parent-build prefill, this build's prefill, this build's score; best of each.  The stepped
alternative (l2z_transformer + l2z_logits_read per position) at 128 tokens only.

Model of the extra cost: the classifier product is 2 P 32000 4096 flop against 2 P (4 4096^2 + 3 4096 11008) per layer,
0.65 of one of the 32 layers, so score - prefill should be near 0.65 x prefill / 32; the acceptance bound is twice that,
with the PARENT build's prefill as "prefill".

    python scripts/score_bench.py [--parent-lib PATH] [--out profiles/score_bench.md] [--sizes 128,512,1024]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/score_bench.py --profile 1024   # the kernel table
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load():
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    return np, pkg.binding, pkg.checkpoint


def tokens_of(np, cfg, n):
    return np.array([1] + np.random.default_rng(n).integers(2, cfg.vocab_size, n - 1).tolist(), np.int32)


def child():
    """Times l2z_prefill of the library L2Z_LIB names: one line in ("prefill N"), one line out (milliseconds)."""
    np, B, ck = load()
    cfg = ck.LLAMA2_7B
    w, s = B.Weights(cfg, None, False, seed=1), B.RunState(cfg)
    print("ready", flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        toks = tokens_of(np, cfg, int(cmd[1]))
        t0 = time.perf_counter()
        s.prefill(toks, 0, w)
        print(f"{(time.perf_counter() - t0) * 1e3:.4f}", flush=True)
    s.close(); w.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.md"))
    ap.add_argument("--sizes", default="128,512,1024")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--profile", type=int, default=0, metavar="N",
                    help="nothing but 3 l2z_score calls of N tokens after one warm-up (the program of a rocprofv3 --kernel-trace run)")
    a = ap.parse_args()
    if a.child:
        return child()
    if a.profile:
        np, B, ck = load()
        cfg = ck.LLAMA2_7B
        w, s = B.Weights(cfg, None, False, seed=1), B.RunState(cfg)
        for _ in range(4):
            s.score(tokens_of(np, cfg, a.profile), 0, w)
        s.close(); w.close()
        return
    kid = None
    if a.parent_lib:   # started before this process touches the GPU
        kid = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], stdin=subprocess.PIPE,
                               stdout=subprocess.PIPE, text=True, env=dict(os.environ, L2Z_LIB=os.path.abspath(a.parent_lib)))
        assert kid.stdout.readline().strip() == "ready", "the child with the parent build did not start"

    def parent_prefill(n):
        if kid is None:
            return float("nan")
        kid.stdin.write(f"prefill {n}\n"); kid.stdin.flush()
        return float(kid.stdout.readline())

    np, B, ck = load()
    cfg = ck.LLAMA2_7B
    w, s = B.Weights(cfg, None, False, seed=1), B.RunState(cfg)
    name = B.device_info(0)[0]

    def timed(f):
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    rows, detail = [], []
    for n in [int(x) for x in a.sizes.split(",")]:
        toks = tokens_of(np, cfg, n)
        for _ in range(2):   # warm-up: allocations, code objects
            parent_prefill(n); s.prefill(toks, 0, w); s.score(toks, 0, w)
        pp, pf, sc = [], [], []
        for _ in range(a.rounds):
            pp.append(parent_prefill(n))
            pf.append(timed(lambda: s.prefill(toks, 0, w)))
            sc.append(timed(lambda: s.score(toks, 0, w)))
        stepped = float("nan")
        if n <= 128:
            def step_all():
                for i, t in enumerate(toks):
                    s.transformer(int(t), i, w)
                    s.logits()
            step_all()
            stepped = min(timed(step_all) for _ in range(2))
        base = min(pp) if kid else min(pf)
        model = 0.65 * base / 32.0
        extra = min(sc) - base
        rows.append((n, min(pp), max(pp), min(pf), min(sc), extra, model, extra / model, stepped))
        detail.append((n, pp, pf, sc))
        print(f"{n:5d} tokens: parent prefill {min(pp):7.2f}..{max(pp):7.2f} ms | prefill {min(pf):7.2f} | score {min(sc):7.2f} | "
              f"score - prefill(parent) {extra:6.2f} ms = {extra / model:4.2f} x model {model:5.2f} | stepped {stepped:8.1f}", flush=True)
    if kid:
        kid.stdin.write("quit\n"); kid.stdin.flush(); kid.wait(timeout=60)
    s.close(); w.close()

    with open(a.out, "w") as f:
        f.write("# l2z_score vs l2z_prefill, Llama-2-7B shape (scripts/score_bench.py)\n\n")
        f.write(f"Device: {name}.  One process per build, alternating; best of {a.rounds} after warm-up; wall-clock ms of the "
                "synchronous calls.  \"parent\": l2z_prefill of the parent commit's build"
                + ("" if kid else " -- not measured (no --parent-lib): this build's prefill stands in") + ".  "
                "Model: 0.65 x prefill / 32 (the classifier product's share of one layer's flop).\n\n")
        f.write("| tokens | parent prefill (best .. worst) | prefill | score | score - parent prefill | model | ratio (bound 2) | stepped + logits read |\n")
        f.write("|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for n, p0, p1, pf, sc, ex, md, ra, st in rows:
            stepped = "not measured" if st != st else f"{st:.1f}"
            parent = "not measured" if p0 != p0 else f"{p0:.2f} .. {p1:.2f}"
            f.write(f"| {n} | {parent} | {pf:.2f} | {sc:.2f} | {ex:.2f} | {md:.2f} | {ra:.2f} | {stepped} |\n")
        f.write("\nAll readings (ms), in round order:\n\n")
        for n, pp, pf, sc in detail:
            f.write(f"* {n} tokens: parent prefill {', '.join(f'{v:.2f}' for v in pp)}; prefill {', '.join(f'{v:.2f}' for v in pf)}; "
                    f"score {', '.join(f'{v:.2f}' for v in sc)}\n")


if __name__ == "__main__":
    main()
