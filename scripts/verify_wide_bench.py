"""l2z_verify_wide (synthetic weights): one call for the speculative rows of many sequences against the loop of
l2z_verify_batch calls over the same sequences -- each call taking as many whole sequences as fit in 16 rows -- and against
l2z_transformer_wide on the same sequences, the cost of a plain step without guesses.

Shapes: the Llama-2-7B dims with seq_len 1024, and the stories110M dims.  Layouts (sequences x rows each): 16 x 4, 32 x 4,
16 x 8, 64 x 2, 8 x 16, every sequence at pos0 = 16 (short) or 500.  All greedy.  Every form is a synchronous call (for
l2z_transformer_wide: out_next is asked for): wall clock, the forms of a layout alternating in one process, --rounds readings
after a warm-up, best .. worst.  The calls rewrite the same KV rows.  A case that was not run is written down as such.

    python scripts/verify_wide_bench.py [--out profiles/verify_wide_bench.md] [--shapes 7b,110m]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/verify_wide_bench.py --profile 16x4
    (--profile LAYOUT: nothing but 4 l2z_verify_wide calls of that layout at --pos on the first shape)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAYOUTS = {"16x4": (16, 4), "32x4": (32, 4), "16x8": (16, 8), "64x2": (64, 2), "8x16": (8, 16)}
CONTEXTS = (16, 500)


def load():
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    return np, pkg.binding, pkg.checkpoint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_wide_bench.md"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--shapes", default="7b,110m")
    ap.add_argument("--profile", choices=tuple(LAYOUTS), default=None)
    ap.add_argument("--pos", type=int, default=16)
    a = ap.parse_args()
    np, B, ck = load()
    c7 = ck.LLAMA2_7B
    shapes = {"7b": ("Llama-2-7B dims, seq_len 1024",
                     ck.Config(c7.dim, c7.hidden_dim, c7.n_layers, c7.n_heads, c7.n_kv_heads, c7.vocab_size, 1024)),
              "110m": ("stories110M dims", ck.STORIES110M)}
    asked = [s for s in a.shapes.split(",") if s]
    fmt = lambda x: f"{min(x):.3f} .. {max(x):.3f}"
    out = [f"# l2z_verify_wide, synthetic weights (scripts/verify_wide_bench.py)\n\nDevice: {B.device_info(0)[0]}.  Wall clock of "
           f"the synchronous calls in milliseconds, the forms of a layout alternating in one process, {a.rounds} readings after a "
           "warm-up, best .. worst; all greedy.  loop: l2z_verify_batch calls over the same sequences, each taking as many whole "
           "sequences as fit in 16 rows; step: one l2z_transformer_wide call on the same sequences (one row each, no guesses).\n"]
    for key, (title, cfg) in shapes.items():
        out.append(f"\n## {title}\n\n")
        if key not in asked:
            out.append("Not run.\n")
            continue
        w = B.Weights(cfg, None, False, seed=1)
        toks = np.random.default_rng(7).integers(2, cfg.vocab_size, cfg.seq_len).astype(np.int32)
        ss = [B.RunState(cfg) for _ in range(64)]
        depth = [-1] * 64   # the history each runstate holds

        def at(pos0s):
            """runstates 0 .. len(pos0s) - 1 holding toks[:pos0] (one prefill per depth, forks for the rest)"""
            for j, p in enumerate(pos0s):
                if depth[j] == p:
                    continue
                src = next((i for i in range(64) if depth[i] == p), None)
                if src is None:
                    ss[j].prefill(toks[:p], 0, w)
                else:
                    B.runstate_fork(ss[j], ss[src], p)
                depth[j] = p
            return ss[:len(pos0s)]

        def forms(pos0s, rows):
            states = at(pos0s)
            n, per = len(states), 16 // rows
            lists = [toks[p:p + rows] for p in pos0s]
            first = np.array([t[0] for t in lists], np.int32)

            def loop():
                for g in range(0, n, per):
                    B.verify_batch(states[g:g + per], lists[g:g + per], pos0s[g:g + per], w)
            return {"wide": lambda: B.verify_wide(states, lists, pos0s, w), "loop": loop,
                    "step": lambda: B.transformer_wide(states, first, pos0s, w)}

        if a.profile:
            n, rows = LAYOUTS[a.profile]
            f = forms([a.pos] * n, rows)
            for _ in range(4):
                f["wide"]()
        else:
            out.append("| layout | pos0 | l2z_verify_wide | loop of l2z_verify_batch | calls | loop / wide | l2z_transformer_wide | "
                       "wide / step |\n|---|---:|---:|---:|---:|---:|---:|---:|\n")
            for pos in CONTEXTS:
                for name, (n, rows) in LAYOUTS.items():
                    f = forms([pos] * n, rows)
                    for g in f.values():
                        g()   # warm-up of every form
                    t = {k: [] for k in f}
                    for _ in range(a.rounds):
                        for k, g in f.items():
                            t0 = time.perf_counter()
                            g()
                            t[k].append((time.perf_counter() - t0) * 1e3)
                    out.append(f"| {name} | {pos} | {fmt(t['wide'])} | {fmt(t['loop'])} | {n // (16 // rows)} | "
                               f"{min(t['loop']) / min(t['wide']):.2f} | {fmt(t['step'])} | {min(t['wide']) / min(t['step']):.2f} |\n")
                    print(out[-1], end="", flush=True)
        for s in ss:
            s.close()
        w.close()
        if a.profile:
            return
    with open(a.out, "w") as f:
        f.write("".join(out))


if __name__ == "__main__":
    main()
