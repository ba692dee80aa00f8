"""What tests/test_gpu_kv8_prefill.py's whole-pass test relies on, checked on the CPU: with int8 KV rows the reference's own
f32 and f64 modes have no position over the parity bar on the shape and seed of tests/kv8_prefill_cases.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_prefill_cases as pc  # noqa: E402
import q8_cases  # noqa: E402


def test_the_two_modes_agree_at_every_position_of_the_prompt_shape():
    ok, dev = q8_cases.position_report(*pc.reference("f32"), *pc.reference("f64"))
    print(f"seed {pc.SEED}: largest deviation between the modes {dev.max():.3e} of the scale")
    assert ok.all(), f"positions over the parity bar: {list(np.flatnonzero(~ok))}"
