"""What tests/test_gpu_q8_prefill_long.py relies on, checked without a GPU: the two long shapes are valid version-2
checkpoints and their token runs in range; on "long64"'s swept seed the two arithmetic modes of tests/ref_q8.py agree
within the parity bar at every one of the 300 positions -- an exception on the device is then the device's summation order
alone --; every (shape, chunk length) the whole-pass tests use keeps the prompt attention on the kernel whose result does
not depend on the chunk; and the GEMM case list holds every situation its table claims."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_prefill_cases as pc  # noqa: E402
import q8_prefill_long_cases as lc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(lc.SHAPES))
def test_the_long_shapes_are_version_2_checkpoints_with_tokens_in_range(ck, name):
    cfg, gs = lc.config(ck, name)
    assert cfg.seq_len == 640 and cfg.n_layers == 2 and cfg.n_heads == 4 and cfg.n_kv_heads == 2
    for g in ((32, 64) if name == "long64" else (gs,)):   # ("long64" is quantized at either size for the scratch's re-make)
        total = ck.v2_layout(cfg, True, g)[-1]
        _, g_, _, body = lc.model(name, gs=g)
        assert g_ == g and len(body) == total and cfg.dim % g == 0 and cfg.hidden_dim % g == 0
    if name == "wide80":
        assert cfg.head_size == 80 and cfg.hidden_dim // gs == 13
    toks = lc.tokens(name, cfg.seq_len)
    assert toks.size == cfg.seq_len and toks.min() >= 2 and toks.max() < cfg.vocab_size
    np.testing.assert_array_equal(lc.tokens(name, 300), toks[:300])
    # every plan's positions lie in the cache (the grow test's calls all start at 0 and take the 20 tokens after its 600)
    assert max(n for _, calls in lc.CHUNK_PLANS.values() for n in calls) + 20 <= cfg.seq_len
    assert all(sum(calls) + 24 <= cfg.seq_len for plan, (_, calls) in lc.CHUNK_PLANS.items() if plan != "c grow")


def test_the_two_modes_agree_at_all_300_positions_of_the_swept_seed():
    z32, k32, v32, m32 = lc.reference("f32")
    ref = lc.reference("f64")
    assert z32.shape[0] == lc.REF_TOKENS == 300 and lc.SEEDS["long64"] == lc.SWEEP["best"]
    flipped, ok, dev = pc.check_rule({p: z32[p] for p in range(z32.shape[0])}, k32, v32, ref)
    margin = min(m32, ref[3])
    print(f"long64, seed {lc.SEEDS['long64']}: 300 positions, largest deviation between the modes {dev.max():.3e} of the scale, "
          f"smallest quantization margin {margin:.3e} of a step")
    assert not flipped and ok.all() and dev.max() < 1e-5
    assert abs(margin - lc.SWEEP["margin"]) < 1e-7   # what the sweep printed for this seed


def test_every_chunk_used_keeps_the_attention_on_the_per_query_kernel(ck):
    """launch_prefill_attention's choice, restated in the cases file: the flash form needs head size 64 or 128, the tiled
    form 128 blocks of (head, 64 queries); neither holds here at any chunk length of any plan (and on "long64" the
    reference run's prefixes)."""
    src = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "prefill_attention.hip")).read()
    # the thresholds restated are the launcher's
    assert "n_heads_model * ((P + 63) / 64) >= 128" in src and "n_heads_model * ((P + 63) / 64) >= 32 && P > 32" in src
    assert re.search(r"flash_blocks && \(head_size == 64 \|\| head_size == 128\)", src)
    assert lc.attention_form(32, 128, 512) == "flash" and lc.attention_form(12, 64, 256) == "flash"
    assert lc.attention_form(32, 80, 512) == "tiled" and lc.attention_form(32, 128, 16) == "query"
    used = set()
    for name in lc.SHAPES:
        cfg, _ = lc.config(ck, name)
        lengths = {P for chunk, calls in lc.CHUNK_PLANS.values() for n in calls for P in lc.chunks_of(chunk, n)}
        if name == "long64":
            lengths |= {p + 1 for p in lc.REF_LOGIT_POSITIONS}
        for P in sorted(lengths):
            assert lc.attention_form(cfg.n_heads, cfg.head_size, P) == "query", (name, P)
            assert cfg.n_heads * ((P + 63) // 64) < 128 and cfg.head_size not in (64, 128)
            used.add(P)
    assert {4, 12, 20, 44, 48, 128, 144, 300, 600} <= used
    # the knob's plans: what one call does with the knob set
    assert lc.chunks_of(144, 300) == [144, 144, 12] and lc.chunks_of(48, 100) == [48, 48, 4]
    assert lc.chunks_of(2048, 600) == [600] and lc.chunks_of(4096, 3000) == [2048, 952] and lc.chunks_of(1, 40) == [16, 16, 8]


def test_the_gemm_cases_cover_what_their_table_claims():
    grids = {case: lc.gemm_grid(case[0], case[1]) for case in lc.GEMM_LONG_CASES}
    for case, (n_tiles, nt, n_tt, last, row_tiles, live) in grids.items():
        assert nt == lc.NT_MAX == 8 and n_tt >= 2, case                      # past one column of blocks, every one
        assert (n_tt, last) == lc.GEMM_LONG_CASES[case], case
        assert case[2] % case[3] == 0 and case[1] % 4 == 0
    g = grids
    # a second column of one tile with one live row; 36 weight rows: the third row tile holds 4
    assert g[(129, 36, 288, 32)][2:] == (2, 1, 3, 1)
    assert g[(144, 100, 768, 64)][0] == 9 and g[(144, 100, 768, 64)][5] == 16   # nine tiles exactly
    assert g[(256, 288, 768, 64)][2:4] == (2, 8)                 # two full columns
    assert g[(257, 4, 4224, 64)][2:4] == (3, 1) and g[(257, 4, 4224, 64)][5] == 1   # one row into a third column
    assert g[(300, 100, 11008, 32)][2:4] == (3, 3) and 11008 // 32 == 344 and -(-344 // (8 * 4)) == 11   # eleven K batches a wave
    assert g[(300, 2816, 288, 32)][4] == 176 and g[(300, 2816, 288, 32)][2] == 3
    assert g[(1024, 36, 4096, 64)][2:4] == (8, 8)                # the default chunk cap
    assert g[(2048, 4, 64, 64)][2:4] == (16, 8) and 2048 == min(max(4096, 16), 2048)   # the largest chunk the knob gives
    assert 64 // 64 == 1   # ... ONE group at n = gs = 64: seven of a block's eight waves take no group
    # last columns of 1, 3 and 8 tiles; both group sizes; a d below one row tile and one that is no multiple of 16
    assert {v[3] for v in grids.values()} == {1, 3, 8}
    assert {c[3] for c in grids} == {32, 64} and any(c[1] < 16 for c in grids) and any(c[1] % 16 for c in grids if c[1] > 16)
