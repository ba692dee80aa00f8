"""l2z_verify_tree on the 7B shape (synthetic weights): one call on a 16-node tree -- chain-shaped, a depth-4 tree that
branches at every level, a star -- against l2z_verify with 16 rows in the same process (the yardstick: that call is
unchanged), and against two l2z_verify calls of 8 rows (what a caller with two candidates makes without the tree).

pos0 = 16 (short) and 2000 (long).  Every form is a synchronous call: wall clock, the forms alternating, --rounds readings
after a warm-up, best .. worst.  The guesses are random, so the verdict accepts nothing and the compaction launch moves no
row; `--accept` plants a path the model agrees with along the bush's branch 0 - 2 - 3 - 5 - 9 first (found by one-row calls), so
that four rows move in every layer.  The calls rewrite the same KV rows.

    python scripts/verify_tree_bench.py [--out profiles/verify_tree_bench.md]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/verify_tree_bench.py --profile bush --pos 2000 --accept
    (--profile TREE: nothing but 4 l2z_verify calls of 16 rows and 4 l2z_verify_tree calls of that tree at --pos)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TREES = {"chain": [-1] + list(range(15)),
         "bush": [-1, 0, 0, 2, 1, 3, 3, 4, 2, 5, 5, 6, 7, 8, 0, 1],
         "star": [-1] + [0] * 15}
BUSH_PATH = [0, 2, 3, 5, 9]
CONTEXTS = (16, 2000)


def load():
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    return np, pkg.binding, pkg.checkpoint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_tree_bench.md"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--profile", choices=tuple(TREES), default=None)
    ap.add_argument("--pos", type=int, default=2000)
    ap.add_argument("--accept", action="store_true")
    a = ap.parse_args()
    np, B, ck = load()
    cfg = ck.LLAMA2_7B
    w = B.Weights(cfg, None, False, seed=1)
    rng = np.random.default_rng(7)
    hist = rng.integers(2, cfg.vocab_size, cfg.seq_len).astype(np.int32)
    s = B.RunState(cfg)

    def tokens_at(pos0, accept):
        """16 pairwise different ids, the history's token at the root; accept: the model's own continuation along BUSH_PATH"""
        s.prefill(hist[:pos0], 0, w)
        toks = rng.choice(np.arange(2, cfg.vocab_size), 16, replace=False).astype(np.int32)
        toks[0] = hist[pos0]
        if accept:
            t = int(toks[0])
            for d in range(1, len(BUSH_PATH)):
                t = int(s.verify([t], pos0 + d - 1, w)[0][0])
                toks[BUSH_PATH[d]] = t
        return toks

    if a.profile:
        toks = tokens_at(a.pos, a.accept and a.profile == "bush")
        for _ in range(4):
            s.verify(toks, a.pos, w)   # the yardstick's launches in the same trace
        for _ in range(4):
            _, path, acc = s.verify_tree(toks, TREES[a.profile], a.pos, w)
        print(f"{a.profile} at {a.pos}: accepted {acc}, path {path.tolist()}")
        s.close()
        w.close()
        return

    def measure(pos0):
        toks = tokens_at(pos0, False)
        planted = tokens_at(pos0, True)
        f = {"verify16": lambda: s.verify(toks, pos0, w),
             "verify8x2": lambda: (s.verify(toks[:8], pos0, w), s.verify(np.concatenate([toks[:1], toks[8:15]]), pos0, w))}
        for name, par in TREES.items():
            f[name] = lambda par=par: s.verify_tree(toks, par, pos0, w)
        f["bush, 4 accepted"] = lambda: s.verify_tree(planted, TREES["bush"], pos0, w)
        assert f["bush, 4 accepted"]()[2] >= 4
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
    out = [f"# l2z_verify_tree, Llama-2-7B shape, synthetic weights (scripts/verify_tree_bench.py)\n\nDevice: {B.device_info(0)[0]}.  "
           f"Wall clock of the synchronous calls in milliseconds, the forms alternating, {a.rounds} readings after a warm-up, "
           "best .. worst.  Every tree has 16 nodes; ratio = the tree call / l2z_verify with 16 rows (best readings).  "
           "2 x 8: two l2z_verify calls of 8 rows.\n\n| pos0 | form | ms | ratio to l2z_verify (16 rows) |\n|---:|---|---:|---:|\n"]
    for pos0 in CONTEXTS:
        t = measure(pos0)
        base = min(t["verify16"])
        for k in ("verify16", "chain", "bush", "bush, 4 accepted", "star", "verify8x2"):
            name = {"verify16": "l2z_verify, 16 rows", "verify8x2": "l2z_verify, 2 x 8 rows"}.get(k, "l2z_verify_tree, " + k)
            out.append(f"| {pos0} | {name} | {fmt(t[k])} | {min(t[k]) / base:.3f} |\n")
            print(out[-1], end="", flush=True)
    out.append("\nNot measured: the acceptance a real text gives the tree drafter (lookup_draft_tree).  The tree holds no real "
               "checkpoint; synthetic weights write no natural text.\n")
    s.close()
    w.close()
    with open(a.out, "w") as f:
        f.write("".join(out))


if __name__ == "__main__":
    main()
