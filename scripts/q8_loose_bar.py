#!/usr/bin/env python3
"""The loose bar of the int8 group-quantized whole-pass tests (tests/q8_cases.py LOOSE), measured on the
CPU: the largest deviation between the two arithmetic modes of tests/ref_q8.py -- f32 in runq.c's order, and float64 --
over a sweep of seeded checkpoints of the tests' three shapes, twelve positions each, as a fraction of the scale (the largest |ref| of a position's logits, of its K rows, of its V rows).  Positions where an activation landed on the other side of a rounding boundary are included: they
are what the bar is for.

    python scripts/q8_loose_bar.py [seeds per shape, default 21] [first seed, default 100]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import q8_cases  # noqa: E402
import ref_q8  # noqa: E402
import __graft_entry__ as ge  # noqa: E402


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    ck = ge.load_package().checkpoint
    worst, n_pos, n_over = 0.0, 0, 0
    for name in ("64", "288", "512"):   # (the shapes the bar was measured on)
        for seed in range(first, first + n_seeds):
            cfg, gs, _, body = q8_cases.model(name, seed)
            toks = q8_cases.tokens(name, seed)
            z32, m32 = ref_q8.run_positions(ck, cfg, body, True, gs, toks, "f32")
            z64, m64 = ref_q8.run_positions(ck, cfg, body, True, gs, toks, "f64")
            P = len(toks)
            ok, dev = q8_cases.position_report(z32, m32.kc[:, :P], m32.vc[:, :P], z64, m64.kc[:, :P], m64.vc[:, :P])
            over = [(p, round(float(dev[p]), 5)) for p in range(P) if not ok[p]]
            n_pos += P
            n_over += len(over)
            worst = max(worst, float(dev.max()))
            # (the smallest distance of any activation quotient of the float64 pass to a rounding boundary: the seeds the
            # tests use are picked for a large one, so that another summation order is unlikely to flip an element)
            print(f"{name:>4} seed {seed}: largest deviation {dev.max():.3e} of the scale, margin {min(m64.margins):.2e}, "
                  f"over the parity bar: {over}", flush=True)
    print(f"{n_pos} positions, {n_over} over the parity bar, largest deviation {worst:.4f} of the scale -> LOOSE = 4 x {worst:.4f}")


if __name__ == "__main__":
    main()
