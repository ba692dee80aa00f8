"""What the paged KV cache is for: at the 7B dims with the model's own seq_len of 2048, 128 contiguous
runstates would reserve 2 x 32 x 2048 x 4096 x 4 B = 2.1 GB each, 275 GB in all -- more than the card has beside 27 GB of
weights.  128 PAGED runstates on a pool of 384 pages (26 GB) take a transformer_wide step.  No ratio is asserted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LLAMA2_7B = dict(dim=4096, hidden_dim=11008, n_layers=32, n_heads=32, n_kv_heads=32, vocab_size=32000, seq_len=2048)


def test_128_sequences_at_seq_len_2048_fit_and_step(gpu, ck):
    cfg = ck.Config(**LLAMA2_7B)
    n, n_pages = 128, 384
    contiguous = 2 * cfg.n_layers * cfg.seq_len * cfg.dim * 4
    assert n * contiguous > 270e9   # 275 GB: with 27 GB of weights and the pass's scratch, more than a 288 GB card
    w = gpu.Weights(cfg, None, False, seed=4)
    pool = gpu.KvPool(cfg, n_pages)
    info = pool.info()
    assert info["page_bytes"] == 2 * cfg.n_layers * cfg.n_kv_heads * 64 * (cfg.dim // cfg.n_heads) * 4   # 67 MB
    assert 25e9 < n_pages * info["page_bytes"] < 27e9
    states = [gpu.RunState(cfg, pool=pool) for _ in range(n)]
    rng = np.random.default_rng(7)
    pos = rng.integers(0, 64, n).astype(np.int32)
    tok = rng.integers(2, cfg.vocab_size, n).astype(np.int32)
    # (rows below a sequence's position are the pool's zeros: finite, as every stale row is)
    ids = gpu.transformer_wide(states, tok, pos, w)
    assert ids.shape == (n,) and ((ids >= 0) & (ids < cfg.vocab_size)).all()
    assert pool.info()["n_free"] == n_pages - n
    assert np.isfinite(states[n - 1].logits()).all()
    for s in states:
        s.close()
    assert pool.info()["n_free"] == n_pages
    pool.close()
    w.close()
