"""The decode pass's launches, counted: which kinds l2z_profile_forward issues per pass for f32 and for int8
group-quantized weights, at a position of the one-block attention form and at one of the split form, and that the pass it
enqueues eagerly leaves the logits the captured pass of l2z_transformer leaves, bit for bit.  One layer walk serves every
weight form (forward.cpp enqueue_forward): a form that took another walk's launches, or attached another form's weights,
shows here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_cases  # noqa: E402

pytestmark = pytest.mark.gpu

SPLIT_POS = 4          # L2Z_ATTN_SPLIT_POS: positions from here on take the split attention form (seq_len is 32)
POSITIONS = (0, 5)     # one block per head / split
TOKEN = 7

# (shape of q8_cases, int8 weights, L2Z_FUSE_SMALL, the one-launch q|k|v + attention form is taken at pos 0)
CASES = [
    ("64", True, 1, False),
    ("288", True, 1, False),    # an MHA model whose runstate has the fused form set: int8 weights never take it
    ("64", False, 1, False),    # GQA: no fused form
    ("288", False, 0, False),
    ("288", False, 1, True),    # the fused form: q|k|v launches only, no attention launch
]


def expected_counts(n_layers, fused):
    return {"qkv": n_layers, "attn": 0 if fused else n_layers, "wo": n_layers, "ffn13": n_layers, "ffn2": n_layers,
            "cls": 1, "argmax": 1, "gather": 0}


@pytest.mark.parametrize("name,q8,fuse,fused_at_0", CASES, ids=[f"{n}-{'q8' if q else 'f32'}-fuse{f}" for n, q, f, _ in CASES])
def test_launches_per_kind_and_the_eager_pass_is_the_captured_pass(gpu, options, name, q8, fuse, fused_at_0):
    cfg, gs, blob, body = q8_cases.model(name)
    options(L2Z_ATTN_SPLIT_POS=SPLIT_POS, L2Z_FUSE_SMALL=fuse)
    w = gpu.Weights.from_q8(cfg, body, True, gs) if q8 else gpu.Weights(cfg, blob, True)
    for pos in POSITIONS:
        s = gpu.RunState(cfg)
        prof = s.profile_forward(TOKEN, pos, w)
        counts = {k: n for k, (_, n) in prof.items()}
        z_eager = s.logits()
        s.close()
        # the split attention form is never part of the fused launch
        want = expected_counts(cfg.n_layers, fused_at_0 and pos < SPLIT_POS)
        print(f"{name} q8={q8} fuse={fuse} pos={pos}: {counts}")
        assert counts == want, f"pos {pos}"
        s = gpu.RunState(cfg)
        s.transformer(TOKEN, pos, w)
        z_graph = s.logits()
        s.close()
        assert np.isfinite(z_eager).all()
        np.testing.assert_array_equal(z_eager.view(np.uint32), z_graph.view(np.uint32), err_msg=f"pos {pos}")
    w.close()
