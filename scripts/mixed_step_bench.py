"""l2z_step_mixed (synthetic weights, the Llama-2-7B dims): ONE call for decoding sequences and newly arrived prompts against
the two calls the same work needs without it -- l2z_prefill_batch for the prompts, then l2z_transformer_wide for the
decoders, on twin runstates.

Cells: `shallow` -- seq_len 256, 64 decoders at positions below 32 and two prompts of 96 rows (the cell
tests/test_gpu_step_mixed_perf.py asserts on) -- and `deep` -- seq_len 1024, 64 decoders at positions 480 .. 520 and two
prompts of 96 rows.  All greedy.  Every form is a synchronous call: wall clock, the forms alternating in one process,
--rounds readings after a warm-up, best .. worst.  The calls rewrite the same KV rows.

    python scripts/mixed_step_bench.py [--out profiles/mixed_step_bench.md] [--cells shallow,deep]
    rocprofv3 --kernel-trace --stats -d DIR -o p -- python scripts/mixed_step_bench.py --profile deep
    (--profile CELL: nothing but 4 l2z_step_mixed calls of that cell; the per-launch times of the two attention launches,
    ragged_attention_flash and wide_attention / wide_combine, are read from the kernel statistics)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CELLS = {"shallow": (256, 0, 32), "deep": (1024, 480, 520)}   # seq_len, the decoders' positions [lo, hi)
N_DEC, N_PROMPTS, ROWS = 64, 2, 96


def load():
    import numpy as np
    import __graft_entry__ as ge
    pkg = ge.load_package()
    return np, pkg.binding, pkg.checkpoint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_step_bench.md"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cells", default="shallow,deep")
    ap.add_argument("--profile", choices=tuple(CELLS), default=None)
    a = ap.parse_args()
    np, B, ck = load()
    c7 = ck.LLAMA2_7B
    asked = [a.profile] if a.profile else [c for c in a.cells.split(",") if c]
    fmt = lambda x: f"{min(x):.3f} .. {max(x):.3f}"
    out = [f"# l2z_step_mixed, synthetic weights, Llama-2-7B dims (scripts/mixed_step_bench.py)\n\nDevice: {B.device_info(0)[0]}.  "
           f"Wall clock of the synchronous calls in milliseconds, the forms alternating in one process, {a.rounds} readings after "
           f"a warm-up, best .. worst; all greedy.  {N_DEC} decoders (one row each) and {N_PROMPTS} prompts of {ROWS} rows from "
           "position 0.  two calls: l2z_prefill_batch for the prompts, then l2z_transformer_wide for the decoders, on twin "
           "runstates.\n\n| cell | seq_len | decoders at | l2z_step_mixed | prefill_batch + transformer_wide | of which prefill_batch "
           "| two calls / mixed |\n|---|---:|---|---:|---:|---:|---:|\n"]
    w = None
    for cell, (seq_len, lo, hi) in CELLS.items():
        if cell not in asked:
            out.append(f"| {cell} | {seq_len} | {lo} .. {hi - 1} | not run | | | |\n")
            continue
        cfg = ck.Config(c7.dim, c7.hidden_dim, c7.n_layers, c7.n_heads, c7.n_kv_heads, c7.vocab_size, seq_len)
        w = B.Weights(cfg, None, False, seed=1)   # (the weights do not depend on seq_len, but a Weights object is made with its config)
        rng = np.random.default_rng(7)
        pos = rng.integers(lo, hi, N_DEC).astype(np.int32)
        tok = rng.integers(2, cfg.vocab_size, N_DEC).astype(np.int32)
        prompts = [np.r_[1, rng.integers(2, cfg.vocab_size, ROWS - 1)].astype(np.int32) for _ in range(N_PROMPTS)]
        mine = [B.RunState(cfg) for _ in range(N_DEC + N_PROMPTS)]
        twins = [] if a.profile else [B.RunState(cfg) for _ in range(N_DEC + N_PROMPTS)]
        if hi > 32:   # a history under the decoders: one prompt pass, forks for the rest
            hist = rng.integers(2, cfg.vocab_size, hi).astype(np.int32)
            mine[0].prefill(hist, 0, w)
            for s in mine[1:N_DEC] + twins[:N_DEC]:
                B.runstate_fork(s, mine[0], hi)
        lists = [[t] for t in tok] + prompts
        pos0 = np.r_[pos, np.zeros(N_PROMPTS, np.int32)].astype(np.int32)
        mixed = lambda: B.step_mixed(mine, lists, pos0, w)
        if a.profile:
            for _ in range(4):
                mixed()
        else:
            pre = lambda: B.prefill_batch(twins[N_DEC:], prompts, 0, w)
            step = lambda: B.transformer_wide(twins[:N_DEC], tok, pos, w)
            for g in (mixed, pre, step):
                g()   # warm-up of every form
            t = {"mixed": [], "pre": [], "two": []}
            for _ in range(a.rounds):
                t0 = time.perf_counter()
                mixed()
                t1 = time.perf_counter()
                pre()
                t2 = time.perf_counter()
                step()
                t3 = time.perf_counter()
                t["mixed"].append((t1 - t0) * 1e3)
                t["pre"].append((t2 - t1) * 1e3)
                t["two"].append((t3 - t1) * 1e3)
            out.append(f"| {cell} | {seq_len} | {lo} .. {hi - 1} | {fmt(t['mixed'])} | {fmt(t['two'])} | {fmt(t['pre'])} | "
                       f"{min(t['two']) / min(t['mixed']):.2f} |\n")
            print(out[-1], end="", flush=True)
        for s in mine + twins:
            s.close()
        w.close()
    if not a.profile:
        with open(a.out, "w") as f:
            f.write("".join(out))


if __name__ == "__main__":
    main()
