"""The recorded oracle pass of tests/test_gpu_wide_decode.py (its widest shape), without a GPU: the file belongs to the plan
the test builds today, and its rows at the shallow positions -- the first segment's edge included -- are what the CPU
oracle computes now, bit for bit (the deep rows cost the oracle a minute: scripts/wide_golden.py)."""
import numpy as np

import test_gpu_wide_decode as T


def test_recorded_pass_matches_the_plan_and_the_oracle(ck, orc):
    for shape, path in T.GOLDEN.items():
        _, prefix, pos, tok = T.plan(ck, shape)
        g = np.load(path)
        assert np.array_equal(g["prefix"], prefix) and np.array_equal(g["pos"], pos) and np.array_equal(g["tok"], tok)
        assert int(g["seed"]) == T.SEED[shape] and g["z"].shape == (T.WIDE, T.SHAPES[shape]["vocab_size"])
        rows = [i for i in range(T.WIDE) if pos[i] <= 65]
        assert {0, 63, 64, 65} <= {int(pos[i]) for i in rows}
        live = T.oracle_rows(ck, orc, shape, rows)
        assert np.array_equal(live.view(np.uint32), g["z"][rows].view(np.uint32))
