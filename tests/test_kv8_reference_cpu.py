"""What tests/test_gpu_kv8.py relies on, checked on the CPU: with int8 KV rows (tests/kv8_cases.py) the reference's own f32
and f64 modes have no position over the parity bar on the shapes and seeds the GPU test uses -- a flipped byte would stay in
the cache and move every later position --."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_cases  # noqa: E402
import q8_cases  # noqa: E402


@pytest.mark.parametrize("name", kv8_cases.SHAPES)
def test_the_two_modes_agree_at_every_position_with_int8_rows(name):
    ok, dev = q8_cases.position_report(*kv8_cases.reference(name, "f32"), *kv8_cases.reference(name, "f64"))
    print(f"shape {name} seed {kv8_cases.SEEDS[name]}: largest deviation between the modes {dev.max():.3e} of the scale")
    assert ok.all(), f"positions over the parity bar: {list(np.flatnonzero(~ok))}"

