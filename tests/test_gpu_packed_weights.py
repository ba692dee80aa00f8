"""The 29-bit packed copy of the W1 | W3 slots that the decode's ffn13 launch streams (csrc/packed_w.h),
on the GPU:

  * every packed slot of the 7B shape decodes on the device to exactly the f32 bits l2z_weights_read returns;
  * 7B decode with the packed copy (L2Z_PACKED_W=1) against the f32 weights (=0): the same greedy tokens and
    bit-identical logits, at short positions and from position 1024 on;
  * slots outside the format (span of 31 binades, a denormal, NaN, Inf) stay f32 -- exactly the ones the numpy rule
    names -- and the results are those of the f32 pass, bit for bit; +-0 and a span of exactly 30 are packed.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu



def np_encodable(m):
    """numpy statement of the format's rule (packed_w.h encodable)."""
    b = np.ascontiguousarray(m, np.float32).view(np.uint32).ravel()
    e = (b >> 23) & 0xFF
    mant = b & 0x7FFFFF
    if np.any(e == 255) or np.any((e == 0) & (mant != 0)):
        return False
    nz = e[e != 0]
    return nz.size == 0 or int(nz.min()) + 30 >= int(nz.max())


def _bind(B):
    L = B.lib()
    L.l2z_weights_packed_count.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.l2z_weights_packed_read.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_size_t]
    return L


def packed_count(B, w):
    L = _bind(B)
    a, b = C.c_int(0), C.c_int(0)
    assert L.l2z_weights_packed_count(w.h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def packed_read(B, w, layer, rows, cols):
    L = _bind(B)
    out = np.empty(rows * cols, np.float32)
    rc = L.l2z_weights_packed_read(w.h, layer, out.ctypes.data_as(C.POINTER(C.c_float)), out.size)
    return rc, out.reshape(rows, cols)


def f32_slot(ck, cfg, w, layer):
    """the f32 W1 | W3 slot the packed one stands for, from l2z_weights_read: W1 / W3 rows interleaved"""
    t = {x.name: x for x in ck.tensor_table(cfg, False)}
    def one(name):
        rows, cols = t[name].shape[-2], t[name].shape[-1]
        return w.read(t[name].offset + layer * rows * cols, rows * cols).reshape(rows, cols)
    a, b = one("w1"), one("w3")
    out = np.empty((2 * a.shape[0], a.shape[1]), np.float32)
    out[0::2], out[1::2] = a, b
    return out


def with_packed(B, value, make):
    B.option_set("L2Z_PACKED_W", value)
    try:
        return make()
    finally:
        B.option_set("L2Z_PACKED_W", 1)


@pytest.fixture(scope="module")
def w7b(gpu, ck):
    cfg = ck.LLAMA2_7B
    w = gpu.Weights(cfg, None, False, seed=2024)
    yield cfg, w
    w.close()


def test_7b_every_slot_is_packed_and_decodes_to_the_f32_bits(gpu, ck, w7b):
    cfg, w = w7b
    assert packed_count(gpu, w) == (cfg.n_layers, cfg.n_layers)
    for layer in range(cfg.n_layers):
        ref = f32_slot(ck, cfg, w, layer)
        assert np_encodable(ref)
        rc, got = packed_read(gpu, w, layer, *ref.shape)
        assert rc == 0, layer
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), layer


def _steps(s, w, tok, pos0, n):
    toks, logits = [], []
    for p in range(pos0, pos0 + n):
        s.transformer(tok, p, w)
        lg = s.logits()
        logits.append(lg.view(np.uint32).copy())
        tok = int(np.argmax(lg))
        toks.append(tok)
    return toks, logits


def test_7b_decode_packed_equals_f32_short_and_long(gpu, ck, w7b):
    cfg, w = w7b
    s_f = with_packed(gpu, 0, lambda: gpu.RunState(cfg))
    s_p = gpu.RunState(cfg)
    # short positions: 64 stepped tokens
    tf, lf = _steps(s_f, w, 1, 0, 64)
    tp, lp = _steps(s_p, w, 1, 0, 64)
    assert tf == tp
    for i, (a, b) in enumerate(zip(lf, lp)):
        assert np.array_equal(a, b), i
    # the captured greedy loop
    s_f.greedy_begin([])
    s_p.greedy_begin([])
    assert np.array_equal(np.asarray(s_f.greedy_run(w, 64)), np.asarray(s_p.greedy_run(w, 64)))
    # long positions: the same 1024-token prompt (f32 prefill in both), then 64 steps from position 1024
    prompt = (np.arange(1024) * 7919 % (cfg.vocab_size - 3) + 3).astype(np.int32)
    s_f.prefill(prompt, 0, w)
    s_p.prefill(prompt, 0, w)
    tf, lf = _steps(s_f, w, 5, 1024, 64)
    tp, lp = _steps(s_p, w, 5, 1024, 64)
    assert tf == tp
    for i, (a, b) in enumerate(zip(lf, lp)):
        assert np.array_equal(a, b), 1024 + i


EDGE = ("zeros_and_span_30", "span_31", "denormal", "nan", "inf")


def _edge_blob(ck, cfg, case):
    rng = np.random.default_rng(7)
    t = {x.name: x for x in ck.tensor_table(cfg, False)}
    blob = np.empty(ck.weights_count(cfg, False), np.float32)
    for x in t.values():
        blob[x.offset:x.offset + x.count] = x.bias + x.scale * rng.uniform(-1, 1, x.count).astype(np.float32)
    def mat(name):
        x = t[name]
        return blob[x.offset:x.offset + x.count].reshape(x.shape[-2], x.shape[-1])
    w1, w3 = mat("w1"), mat("w3")
    e_max = int(((np.concatenate([w1.ravel(), w3.ravel()]).view(np.uint32) >> 23) & 0xFF).max())
    if case == "zeros_and_span_30":
        w1[0, :8] = 0.0
        w3[1, :8] = -0.0
        w1[2, 3] = -np.float32(2.0) ** (e_max - 30 - 127)
    elif case == "span_31":
        w3[5, 7] = np.float32(2.0) ** (e_max - 31 - 127)
    elif case == "denormal":
        w1[9, 9] = np.float32(-3e-39)
    elif case == "nan":
        w3[17, 1] = np.float32(np.nan)
    else:
        w1[18, 2] = np.float32(np.inf)
    return blob


@pytest.mark.parametrize("case", EDGE)
def test_edge_cases_pack_or_take_the_f32_fallback_with_identical_results(gpu, ck, case):
    cfg = ck.Config(4096, 4096, 1, 32, 32, 512, 64)
    w = gpu.Weights(cfg, _edge_blob(ck, cfg, case), False)
    try:
        ref = f32_slot(ck, cfg, w, 0)
        want = case == "zeros_and_span_30"
        assert np_encodable(ref) == want
        assert packed_count(gpu, w) == (int(want), 1)
        rc, got = packed_read(gpu, w, 0, *ref.shape)
        if want:
            assert rc == 0
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        else:
            assert rc != 0
        s_f = with_packed(gpu, 0, lambda: gpu.RunState(cfg))
        s_p = gpu.RunState(cfg)
        tf, lf = _steps(s_f, w, 1, 0, 16)
        tp, lp = _steps(s_p, w, 1, 0, 16)
        assert tf == tp
        for i, (a, b) in enumerate(zip(lf, lp)):
            assert np.array_equal(a, b), i
    finally:
        w.close()


def test_knob_zero_builds_no_packed_copy(gpu, ck):
    cfg = ck.Config(4096, 4096, 1, 32, 32, 512, 64)
    w = with_packed(gpu, 0, lambda: gpu.Weights(cfg, None, False, seed=3))
    try:
        assert packed_count(gpu, w) == (0, 0)
        rc, _ = packed_read(gpu, w, 0, 8192, 4096)
        assert rc != 0
    finally:
        w.close()
