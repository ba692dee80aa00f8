"""What tests/test_gpu_q8_batch.py relies on, checked where it is cheap (no GPU): the shapes of tests/q8_batch_cases.py hold
the edges they were picked for, the verify cases lie where they are said to lie, the reference runs are
tests/q8_prefill_cases.py's -- on which the two arithmetic modes of tests/ref_q8.py agree at the parity bar at EVERY
position, so an exception on the device is the device's summation order alone --, and the numpy embedding rows are the
reference's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import q8_batch_cases as bc  # noqa: E402
import q8_cases  # noqa: E402
import q8_prefill_cases as pc  # noqa: E402
import q8_prefill_long_cases as lc  # noqa: E402


def test_the_exact_shapes_hold_their_edges():
    assert bc.KV24 == (96, 256, 2, 4, 1, 260, 160, 32)
    cfg, gs, _, _ = bc.model("kv24")
    assert cfg.head_size == 24 and cfg.kv_dim == 24 and cfg.head_size % 4 == 0
    # six full tiles of q, then K and V segments of one and a half tiles each
    assert bc.qkv_tiles("kv24") == (6, 2, 16, 8)
    assert cfg.vocab_size % 4 == 0 and cfg.vocab_size % bc.TILE == 4
    assert cfg.seq_len == 160 and -(-cfg.seq_len // bc.SEG) == 3
    # three and eight groups a row: five, and none, of the eight waves of a block get no group
    assert cfg.dim // gs == 3 and cfg.hidden_dim // gs == 8
    cfg, gs, _, _ = bc.model("wide80")
    assert (cfg.head_size, gs, cfg.seq_len) == (80, 64, 640) and cfg.n_heads != cfg.n_kv_heads
    assert bc.model("wide80")[3] is lc.model("wide80")[3] and bc.model("64")[3] is q8_cases.model("64")[3]
    for name in bc.EXACT_SHAPES + tuple(bc.REFERENCE_CALLS):
        cfg = bc.model(name)[0]
        assert cfg.head_size % 4 == 0 and cfg.head_size <= 256 and cfg.vocab_size % 4 == 0, name
        assert tuple(int(v) for v in cfg.as_i32()) == bc.shape(name)[:7]


def test_the_verify_cases_lie_where_they_are_said_to():
    seen = set()
    for name, pos0, n in bc.VERIFY_CASES:
        cfg = bc.model(name)[0]
        assert 1 <= n <= bc.BATCH_MAX and pos0 + n <= cfg.seq_len
        assert bc.tokens(name).size >= pos0 + n
        seen.add((name, pos0))
    assert seen == {("64", 0), ("kv24", 0), ("kv24", 60), ("wide80", 130)}
    assert {n for _, _, n in bc.VERIFY_CASES} == {2, 8, 16}
    # from position 60 the calls of 8 and 16 rows have rows on both sides of the boundary between segments 0 and 1 ...
    for n in (8, 16):
        assert 60 // bc.SEG == 0 and (60 + n - 1) // bc.SEG == 1
    # ... and from 130 every row reads three segments, the last one partly
    assert 130 // bc.SEG == 2 and 145 // bc.SEG == 2


def test_the_reference_calls_cover_the_prefill_runs():
    for name, calls in bc.REFERENCE_CALLS.items():
        assert sum(calls) == pc.RUN_LENGTH[name] and all(1 <= n <= bc.BATCH_MAX for n in calls)
        np.testing.assert_array_equal(bc.tokens(name), pc.tokens(name))
        assert pc.RUN_LENGTH[name] >= bc.BATCH_REF_STEPS
        feeds = bc.batch_feeds(name)
        V = bc.model(name)[0].vocab_size
        assert feeds.shape == (3, bc.BATCH_REF_STEPS) and feeds.min() >= 2 and feeds.max() < V
        np.testing.assert_array_equal(feeds[0], pc.tokens(name)[:bc.BATCH_REF_STEPS])
        assert not np.array_equal(feeds[1], feeds[0]) and not np.array_equal(feeds[2], feeds[0])


@pytest.mark.parametrize("name", list(bc.REFERENCE_CALLS))
def test_the_two_modes_agree_on_every_reference_run(name):
    z32, k32, v32, _ = pc.reference(name, "f32")
    ref = pc.reference(name, "f64")
    flipped, ok, dev = pc.check_rule({p: z32[p] for p in range(z32.shape[0])}, k32, v32, ref)
    print(f"shape {name}: largest deviation between the modes {dev.max():.3e} of the scale")
    assert not flipped and ok.all() and dev.max() < 1e-5


def test_the_numpy_embedding_rows_are_the_reference_s(ck):
    cfg, gs, _, body = bc.model("kv24")
    t = ck.v2_carve(cfg, body, True, gs)
    eq, es = t["token_embedding_table"]
    toks = bc.tokens("kv24", 5)
    rows = bc.embedding_rows(eq[0], es[0].reshape(cfg.vocab_size, -1), toks, gs)
    for r, tok in zip(rows, toks):
        want = (eq[0, tok].astype(np.float32) * np.repeat(es[0, tok], gs)).astype(np.float32)   # ref_q8.Q8Model.transformer's
        np.testing.assert_array_equal(r.view(np.uint32), want.view(np.uint32))
