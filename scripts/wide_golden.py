#!/usr/bin/env python3
"""Writes the recorded oracle pass tests/test_gpu_wide_decode.py reads for its widest shape (GOLDEN there): the CPU oracle's
logits of all 128 rows of that shape's plan, with the plan beside them.  No GPU; about a minute.

  python scripts/wide_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import test_gpu_wide_decode as T  # noqa: E402


def main():
    ck, orc = ge.load_package().checkpoint, ge.load_oracle()
    for shape, path in T.GOLDEN.items():
        _, prefix, pos, tok = T.plan(ck, shape)
        z = T.oracle_rows(ck, orc, shape, list(range(T.WIDE)))
        np.savez_compressed(path, z=z, prefix=prefix, pos=pos, tok=tok, seed=np.int64(T.SEED[shape]))
        print(f"{shape}: {z.shape} -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
