"""Interleaved A/B of BUILDS of the library on the batched prompt pass -- prefill_ab.py's method with the library switched per
process (L2Z_LIB) instead of a knob per call: every round runs one child process per build, the order rotating from round to
round, and a child times s.prefill at 64, 128, 512 and 1024 tokens with L2Z_PF_X3 1 and 0 (one untimed pass, then the median
of REPS).  Give the parent's build twice (two separate builds) and the head's: the difference between the two parent builds is
the noise floor.
Per point and round i: d_AA_i = parent2_i - parent_i, d_AB_i = head_i - parent_i; the spread is max_i |d_AA_i| and the head
lies inside it where |median_i d_AB_i| <= spread.  A child that fails or runs out of time ends the run: nothing is started
behind it.

usage: python scripts/prefill_lib_ab.py <shape> <rounds> <parent .so> <parent2 .so> <head .so>"""
import json, os, subprocess, sys, time

POINTS = [(n, x3) for x3 in (1, 0) for n in (64, 128, 512, 1024)]
REPS = 7


def child(shape):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import numpy as np, __graft_entry__ as ge
    pkg = ge.load_package(); B, ck = pkg.binding, pkg.checkpoint
    cfg, shared = {k: (c, sh) for k, c, sh in ck.iter_configs()}[shape]
    w = B.Weights(cfg, None, shared, seed=1); s = B.RunState(cfg)
    out = {}
    for n, x3 in POINTS:
        toks = [1] + np.random.default_rng(1).integers(2, cfg.vocab_size, n - 1).tolist()
        B.option_set("L2Z_PF_X3", x3)
        ts = []
        for r in range(REPS + 1):
            t0 = time.perf_counter(); s.prefill(toks, 0, w); dt = time.perf_counter() - t0   # (ends in a stream synchronise)
            if r > 0: ts.append(dt)
        out[f"{n} tokens, L2Z_PF_X3={x3}"] = float(np.median(ts)) * 1e3
    B.option_set("L2Z_PF_X3", 1)
    print(json.dumps(out), flush=True)


def main():
    shape, rounds, libs = sys.argv[1], int(sys.argv[2]), sys.argv[3:]
    assert len(libs) == 3, "parent, parent2, head"
    res = [[] for _ in libs]   # [lib][round] -> {point: ms}
    for r in range(rounds):
        for i in [(r + j) % len(libs) for j in range(len(libs))]:   # (the order rotates: a box that warms up during a round favours no build)
            lib = libs[i]
            p = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--child", shape],
                               env=dict(os.environ, L2Z_LIB=os.path.abspath(lib)), capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit(f"round {r}, {lib}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            res[i].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"round {r} {lib}: {res[i][-1]}", flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2] if len(xs) % 2 else sum(sorted(xs)[len(xs) // 2 - 1: len(xs) // 2 + 1]) / 2
    print("| point | parent ms | parent2 ms | head ms | A/A spread ms | median head - parent ms | inside |\n|---|---:|---:|---:|---:|---:|---|")
    for n, x3 in POINTS:
        k = f"{n} tokens, L2Z_PF_X3={x3}"
        a, a2, h = ([res[i][r][k] for r in range(rounds)] for i in range(3))
        spread = max(abs(y - x) for x, y in zip(a, a2))
        d = med([y - x for x, y in zip(a, h)])
        print(f"| {k} | {med(a):.3f} | {med(a2):.3f} | {med(h):.3f} | {spread:.3f} | {d:+.3f} | {'yes' if abs(d) <= spread else 'NO'} |")


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
