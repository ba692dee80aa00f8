"""l2z_prefill_batch against the loop of l2z_prefill over the same sequences, on the 7B shape.

One process, one set of weights, 16 runstates.  Per layout, after a warm-up of both legs, 6 rounds of: the loop (one
l2z_prefill per sequence, then a synchronize of every runstate), the batch call (then the same synchronizes); wall-clock
ms, best of each and every reading.  Both legs rewrite the same KV rows of the same runstates.

    python scripts/prefill_batch_bench.py [--out profiles/prefill_batch_bench.md] [--kernel-table TABLE.md]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/prefill_batch_bench.py --profile   # ONE 16 x 32 call, nothing else
    python scripts/rocprof_summary.py DIR/.../p_results.db "<label>" > TABLE.md

--kernel-table: the table of such a profiler run, appended to the report (32 layers: 32 ragged_attention_* launches and 32
ragged_rope_scatter launches in the one call; the weights' generation is in the table too).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYOUTS = [("16 x 32", [32] * 16), ("16 x 64", [64] * 16), ("8 x 128", [128] * 8), ("16 x 100 (three chunks)", [100] * 16),
           ("4 x 512", [512] * 4), ("mixed 5 ... 200", [5, 200, 18, 131, 64, 33, 97, 150, 8, 76, 41, 180, 25, 112, 57, 90])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_batch_bench.md"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--profile", action="store_true", help="ONE 16 x 32 l2z_prefill_batch call, nothing else")
    ap.add_argument("--kernel-table", default=None)
    a = ap.parse_args()
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    B, ck = pkg.binding, pkg.checkpoint
    cfg = ck.LLAMA2_7B
    w = B.Weights(cfg, None, False, seed=1)
    states = [B.RunState(cfg) for _ in range(16)]
    rng = np.random.default_rng(3)

    def lists_of(lengths):
        return [np.array([1] + rng.integers(2, cfg.vocab_size, n - 1).tolist(), np.int32) for n in lengths]

    def sync(ss):
        for s in ss:
            s.synchronize()

    if a.profile:
        ls = lists_of([32] * 16)
        B.prefill_batch(states, ls, 0, w)
        sync(states)
        return
    name = B.device_info(0)[0]
    rows = []
    for label, lengths in LAYOUTS:
        ss, ls = states[:len(lengths)], lists_of(lengths)

        def loop():
            for s, t in zip(ss, ls):
                s.prefill(t, 0, w)
            sync(ss)

        def batch():
            B.prefill_batch(ss, ls, 0, w)
            sync(ss)

        def timed(f):
            t0 = time.perf_counter()
            f()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(2):
            loop(); batch()
        tl, tb = [], []
        for _ in range(a.rounds):
            tl.append(timed(loop)); tb.append(timed(batch))
        rows.append((label, sum(lengths), tl, tb))
        print(f"{label:24s} {sum(lengths):5d} rows: loop {min(tl):8.2f} ms | batch {min(tb):8.2f} ms | {min(tl) / min(tb):5.2f} x", flush=True)
    for s in states:
        s.close()
    w.close()
    with open(a.out, "w") as f:
        f.write("# l2z_prefill_batch vs the loop of l2z_prefill, Llama-2-7B shape (scripts/prefill_batch_bench.py)\n\n")
        f.write(f"Device: {name}.  One process, both legs alternating; best of {a.rounds} after a warm-up; wall-clock ms of the calls plus a "
                "synchronize of every runstate.\n\n")
        f.write("| layout | rows | loop of l2z_prefill | l2z_prefill_batch | loop / batch |\n|---|---:|---:|---:|---:|\n")
        for label, n, tl, tb in rows:
            f.write(f"| {label} | {n} | {min(tl):.2f} | {min(tb):.2f} | {min(tl) / min(tb):.2f} |\n")
        f.write("\nAll readings (ms), in round order:\n\n")
        for label, n, tl, tb in rows:
            f.write(f"* {label}: loop {', '.join(f'{v:.2f}' for v in tl)}; batch {', '.join(f'{v:.2f}' for v in tb)}\n")
        if a.kernel_table:
            f.write("\n## One 16 x 32 call under rocprofv3 (`prefill_batch_bench.py --profile`; 32 layers, one chunk of 512 rows)\n\n")
            f.write(open(a.kernel_table).read().replace("# rocprofv3", "rocprofv3", 1))


if __name__ == "__main__":
    main()
