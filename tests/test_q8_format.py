"""llama2.c version-2 checkpoints (int8 group-quantized weights) on the Python side, without a GPU: the
header bytes, a write / read round trip, the weight rule on hand-computed groups, and the layout's totals."""
import struct

import numpy as np
import pytest

f32 = np.float32


def test_header_bytes_literally(ck):
    cfg = ck.Config(64, 192, 2, 4, 2, 512, 32)
    h = ck.v2_header(cfg, True, 32)
    assert len(h) == 256
    assert h[0:4] == bytes([0x32, 0x34, 0x6B, 0x61])            # u32 0x616b3432, little endian: "24ka"
    assert h[4:8] == struct.pack("<i", 2)
    assert h[8:36] == struct.pack("<7i", 64, 192, 2, 4, 2, 512, 32)
    assert h[36] == 1
    assert h[37:41] == struct.pack("<i", 32)                     # unaligned
    assert h[41:] == bytes(215)
    h = ck.v2_header(cfg, False, 64)
    assert h[36] == 0 and h[37:41] == bytes([64, 0, 0, 0])


def test_quantize_q80_on_a_hand_computed_group(ck):
    """max 127 * 2^-2: the scale is exactly 0.25, so these quotients are exact -- ties go to EVEN."""
    v = np.zeros(32, f32)
    v[:12] = np.array([127, -127, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, 125.5, 0.49, 3.25], f32) * f32(0.25)
    q, s = ck.quantize_q80(v, 32)
    assert s.dtype == np.float32 and s.tolist() == [0.25]
    assert q.dtype == np.int8
    assert q[:12].tolist() == [127, -127, 0, 2, 2, 0, -2, -2, 126, 126, 0, 3]
    assert not q[12:].any()


def test_quantize_q80_scale_is_one_f32_division_and_zero_groups_are_zero(ck):
    rng = np.random.default_rng(1)
    w = rng.standard_normal((6, 64)).astype(f32)
    w[2] = 0            # an all-zero group at gs 64, two at gs 32
    w[4, :32] = 0
    for gs in (32, 64):
        q, s = ck.quantize_q80(w, gs)
        assert q.shape == w.shape and s.shape == (w.size // gs,)
        g = w.reshape(-1, gs)
        for i in range(g.shape[0]):
            m = f32(np.abs(g[i]).max())
            assert s[i] == f32(m / f32(127.0))
            if m == 0:
                assert s[i] == 0 and not q.reshape(-1, gs)[i].any()
            else:
                want = [int(np.rint(f32(f32(x) / s[i]))) for x in g[i]]
                assert q.reshape(-1, gs)[i].tolist() == want
        assert np.abs(q).max() == 127


def test_write_read_round_trip(ck, tmp_path):
    cfg = ck.Config(64, 192, 2, 4, 2, 512, 32)
    for shared, gs in ((True, 32), (False, 64)):
        blob = ck.synth_blob(cfg, shared, 3)
        body = ck.v2_body_from_f32(cfg, blob, shared, gs)
        lay = ck.v2_layout(cfg, shared, gs)
        assert body.size == lay.total and ("wcls" in lay.tensors) == (not shared)
        path = tmp_path / f"m{gs}.bin"
        ck.write_checkpoint_v2(path, cfg, body, shared, gs)
        assert path.stat().st_size == 256 + lay.total
        cfg2, shared2, gs2, body2 = ck.read_checkpoint_v2(path)
        assert (cfg2, shared2, gs2) == (cfg, shared, gs)
        assert isinstance(body2, np.memmap) and np.array_equal(np.asarray(body2), body)
        t32, t = ck.carve(cfg, blob, shared), ck.v2_carve(cfg2, body2, shared2, gs2)
        assert np.array_equal(t["rms_att_weight"], t32["rms_att_weight"])
        assert np.array_equal(t["rms_final_weight"], t32["rms_final_weight"])
        for name in ("token_embedding_table", "wq", "wk", "w2", "w3", "wcls"):
            q, s = ck.quantize_q80(t32[name], gs)
            assert np.array_equal(t[name][0].reshape(-1), q.reshape(-1)) and np.array_equal(t[name][1].reshape(-1), s)
        # the file's order: the token embedding first, then wq of every layer, ... w3, then wcls
        offs = [lay.tensors[n].q_offset for n in ck.V2_QUANTIZED if n in lay.tensors]
        assert offs == sorted(offs) and offs[0] == 4 * (2 * cfg.n_layers * cfg.dim + cfg.dim)
    with open(path, "r+b") as f:   # not a version-2 file
        f.write(b"\0")
    with pytest.raises(ValueError):
        ck.read_checkpoint_v2(path)


def test_layout_totals_of_the_named_shapes(ck):
    def by_hand(c, shared, gs):
        values = c.vocab_size * c.dim * (1 if shared else 2) + c.n_layers * (2 * c.dim * c.dim + 2 * c.kv_dim * c.dim + 3 * c.hidden_dim * c.dim)
        return 4 * (2 * c.n_layers * c.dim + c.dim) + values + 4 * (values // gs)

    for name, cfg, shared in ck.iter_configs():
        assert ck.v2_layout(cfg, shared, 32).total == by_hand(cfg, shared, 32), name
    # in bytes: what a 7B version-2 file weighs against 26.4 GB of f32 matrices a token
    assert ck.v2_layout(ck.STORIES15M, True, 32).total == 17_101_440
    assert ck.v2_layout(ck.STORIES42M, True, 32).total == 46_925_824
    assert ck.v2_layout(ck.STORIES110M, True, 64).total == 116_431_872
    assert ck.v2_layout(ck.LLAMA2_7B, False, 64).total == 7_160_348_672
    for cfg, gs in ((ck.STORIES15M, 64), (ck.STORIES42M, 64), (ck.STORIES15M, 16), (ck.LLAMA2_7B, 128)):
        with pytest.raises(ValueError):
            ck.v2_layout(cfg, True, gs)
