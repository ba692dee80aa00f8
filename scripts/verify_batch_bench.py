"""l2z_verify_batch on the 7B shape (synthetic weights): one call for the speculative rows of several sequences against the
loop of l2z_verify calls over the same sequences, and -- with one row per sequence -- against l2z_transformer_batch.

Layouts (sequences x rows each): 4 x 4, 2 x 8, 8 x 2, 16 x 1, every sequence at pos0 = 16 (short) or 2000 (long), and one
mixed-depth layout: 16 x 1 with one sequence at pos 2000 and fifteen at pos 10 (the attention grid's worst case: most blocks
of the (heads, segments, groups) grid are empty).  Every form is a synchronous call (or, for l2z_transformer_batch, the call
and a synchronize): wall clock, the forms of a layout alternating, --rounds readings after a warm-up, best .. worst.  The
calls rewrite the same KV rows.

    python scripts/verify_batch_bench.py [--out profiles/verify_batch_bench.md]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/verify_batch_bench.py --profile mixed
    (--profile LAYOUT: nothing but 4 l2z_verify_batch calls of that layout at --pos)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAYOUTS = {"4x4": (4, 4), "2x8": (2, 8), "8x2": (8, 2), "16x1": (16, 1)}
CONTEXTS = (16, 2000)
MIXED = [2000] + [10] * 15


def load():
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    return np, pkg.binding, pkg.checkpoint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch_bench.md"))
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--profile", choices=tuple(LAYOUTS) + ("mixed",), default=None)
    ap.add_argument("--pos", type=int, default=2000)
    a = ap.parse_args()
    np, B, ck = load()
    cfg = ck.LLAMA2_7B
    w = B.Weights(cfg, None, False, seed=1)
    toks = np.random.default_rng(7).integers(2, cfg.vocab_size, cfg.seq_len).astype(np.int32)
    ss = [B.RunState(cfg) for _ in range(16)]
    depth = [-1] * 16   # the history each runstate holds

    def at(pos0s):
        """runstates 0 .. len(pos0s) - 1 holding toks[:pos0] (one prefill per depth, forks for the rest)"""
        for j, p in enumerate(pos0s):
            if depth[j] == p:
                continue
            src = next((i for i in range(16) if depth[i] == p), None)
            if src is None:
                ss[j].prefill(toks[:p], 0, w)
            else:
                B.runstate_fork(ss[j], ss[src], p)
            depth[j] = p
        return ss[:len(pos0s)]

    def forms(pos0s, rows):
        states = at(pos0s)
        lists = [toks[p:p + rows] for p in pos0s]
        out = {"batch": lambda: B.verify_batch(states, lists, pos0s, w),
               "loop": lambda: [s.verify(t, p, w) for s, t, p in zip(states, lists, pos0s)]}
        if rows == 1:
            def step():
                B.transformer_batch(states, [int(t[0]) for t in lists], pos0s, w)
                states[0].synchronize()
            out["step"] = step
        return out

    if a.profile:
        n, rows = LAYOUTS.get(a.profile, (16, 1))
        f = forms(MIXED if a.profile == "mixed" else [a.pos] * n, rows)
        for _ in range(4):
            f["batch"]()
        for s in ss:
            s.close()
        w.close()
        return

    def measure(pos0s, rows):
        f = forms(pos0s, rows)
        for g in f.values():
            g()   # warm-up of every form
        t = {k: [] for k in f}
        for _ in range(a.rounds):
            for k, g in f.items():
                t0 = time.perf_counter()
                g()
                t[k].append((time.perf_counter() - t0) * 1e3)
        return t

    fmt = lambda x: f"{min(x):.3f} .. {max(x):.3f}"
    out = [f"# l2z_verify_batch, Llama-2-7B shape, synthetic weights (scripts/verify_batch_bench.py)\n\nDevice: {B.device_info(0)[0]}.  "
           f"Wall clock of the synchronous calls in milliseconds, the forms of a layout alternating, {a.rounds} readings after a "
           "warm-up, best .. worst.  loop: one l2z_verify call per sequence; step: l2z_transformer_batch and a synchronize "
           "(one row per sequence only).\n\n| layout | pos0 | l2z_verify_batch | loop of l2z_verify | loop / batch | "
           "l2z_transformer_batch | step / batch |\n|---|---:|---:|---:|---:|---:|---:|\n"]
    cases = [(name, [pos] * n, rows, str(pos)) for pos in CONTEXTS for name, (n, rows) in LAYOUTS.items()]
    cases.append(("16x1 mixed", MIXED, 1, "2000, 15 x 10"))
    for name, pos0s, rows, where in cases:
        t = measure(pos0s, rows)
        step = f"{fmt(t['step'])} | {min(t['step']) / min(t['batch']):.2f}" if "step" in t else "|"
        out.append(f"| {name} | {where} | {fmt(t['batch'])} | {fmt(t['loop'])} | {min(t['loop']) / min(t['batch']):.2f} | {step} |\n")
        print(out[-1], end="", flush=True)
    for s in ss:
        s.close()
    w.close()
    with open(a.out, "w") as f:
        f.write("".join(out))


if __name__ == "__main__":
    main()
