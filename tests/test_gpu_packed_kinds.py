"""The packed copy of every kind of decode row launch (q|k|v, Wo, W1 | W3, W2, the classifier; csrc/packed_w.h, DESIGN.md
4.9), on one-layer models of the smallest widths that reach every path of the row kernel:

  * every packed slot of every kind decodes on the device to exactly the f32 bits l2z_weights_read returns;
  * decode with the packed copy -- all kinds, and each kind alone (L2Z_PACKED_KINDS) -- against the f32 weights
    (L2Z_PACKED_W=0): bit-identical logits over 16 stepped positions and the same 16 greedy tokens;
  * a slot outside the format (a span of 31 binades, a NaN) in Wk, Wo, W2 or the classifier alone makes exactly that
    kind's slot report not packed, leaves the W1 | W3 count alone, and the results are those of the f32 pass.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ("qkv", "wo", "ffn13", "ffn2", "cls")

SHAPES = {
    "gqa_partial_w2": ((4096, 11008, 1, 32, 8, 512, 64), False),    # Wk / Wv of 1024 rows; W2's rows end inside a batch
    "empty_wave_tail": ((4096, 4352, 1, 32, 32, 512, 64), False),   # W2: the last batch gives wave 0 one step, waves 1-3 none
    "two_batch_rows": ((8192, 4096, 1, 64, 64, 512, 64), False),    # two-batch rows for q|k|v, Wo and the classifier
    "shared_embeddings": ((4096, 4096, 1, 32, 32, 512, 64), True),  # the classifier's copy is one of the embedding table
    "odd_vocab": ((4096, 4096, 1, 32, 8, 513, 64), False),          # 513 classifier rows: no pairs to pack
}


def _lib(B):
    L = B.lib()
    L.l2z_weights_packed_count.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.l2z_weights_packed_count_kind.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.l2z_weights_packed_read_kind.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_size_t]
    return L


def count_kind(B, w, kind):
    a, b = C.c_int(0), C.c_int(0)
    assert _lib(B).l2z_weights_packed_count_kind(w.h, B.KINDS.index(kind), C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def count_w13(B, w):
    a, b = C.c_int(0), C.c_int(0)
    assert _lib(B).l2z_weights_packed_count(w.h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def read_kind(B, w, kind, layer, slot, rows, cols):
    out = np.empty(rows * cols, np.float32)
    rc = _lib(B).l2z_weights_packed_read_kind(w.h, B.KINDS.index(kind), layer, slot, out.ctypes.data_as(C.POINTER(C.c_float)), out.size)
    return rc, out.reshape(rows, cols)


def f32_slots(ck, cfg, shared, w):
    """(kind, slot) -> the f32 rows the packed slot stands for, from l2z_weights_read"""
    t = {x.name: x for x in ck.tensor_table(cfg, shared)}

    def one(name):
        rows, cols = t[name].shape[-2], t[name].shape[-1]
        return w.read(t[name].offset, rows * cols).reshape(rows, cols)
    w1, w3 = one("w1"), one("w3")
    w13 = np.empty((2 * w1.shape[0], w1.shape[1]), np.float32)
    w13[0::2], w13[1::2] = w1, w3
    return {("qkv", 0): one("wq"), ("qkv", 1): one("wk"), ("qkv", 2): one("wv"), ("wo", 0): one("wo"), ("ffn13", 0): w13,
            ("ffn2", 0): one("w2"), ("cls", 0): one("token_embedding_table" if shared else "wcls")}


def runstate(B, cfg, packed_w=1, kinds=-1):
    B.option_set("L2Z_PACKED_W", packed_w)
    B.option_set("L2Z_PACKED_KINDS", kinds)
    try:
        return B.RunState(cfg)
    finally:
        B.option_set("L2Z_PACKED_W", 1)
        B.option_set("L2Z_PACKED_KINDS", -1)


def decode(s, w, n=16):
    """logits of n stepped positions (as bits) and n tokens of the captured greedy loop"""
    tok, logits = 1, []
    for p in range(n):
        s.transformer(tok, p, w)
        lg = s.logits()
        logits.append(lg.view(np.uint32).copy())
        tok = int(np.argmax(np.nan_to_num(lg, nan=-np.inf)))
    s.greedy_begin([])
    return np.stack(logits), np.asarray(s.greedy_run(w, n))


@pytest.fixture(scope="module", params=list(SHAPES))
def model(request, gpu, ck):
    dims, shared = SHAPES[request.param]
    cfg = ck.Config(*dims)
    w = gpu.Weights(cfg, None, shared, seed=11)
    ref = decode(runstate(gpu, cfg, packed_w=0), w)   # the f32 pass, once per shape
    yield request.param, cfg, shared, w, ref
    w.close()


def test_every_packed_slot_decodes_to_the_f32_bits(gpu, ck, model):
    name, cfg, shared, w, _ = model
    ref = f32_slots(ck, cfg, shared, w)
    want = {"qkv": (3, 3), "wo": (1, 1), "ffn13": (1, 1), "ffn2": (1, 1), "cls": (1, 1)}
    if name == "odd_vocab":
        want["cls"] = (0, 1)
    for kind in KINDS:
        assert count_kind(gpu, w, kind) == want[kind], kind
    assert count_w13(gpu, w) == (1, 1)
    assert count_kind(gpu, w, "attn") == (0, 0)
    for (kind, slot), m in ref.items():
        rc, got = read_kind(gpu, w, kind, 0, slot, *m.shape)
        if want[kind][0] == 0:
            assert rc != 0, (kind, slot)
            continue
        assert rc == 0, (kind, slot)
        assert np.array_equal(got.view(np.uint32), m.view(np.uint32)), (kind, slot)


def test_decode_equals_f32_with_all_kinds_and_with_each_kind_alone(gpu, model):
    name, cfg, shared, w, (ref_logits, ref_toks) = model
    for mask in [-1] + [1 << gpu.KINDS.index(k) for k in KINDS]:
        logits, toks = decode(runstate(gpu, cfg, kinds=mask), w)
        assert np.array_equal(logits, ref_logits), mask
        assert np.array_equal(toks, ref_toks), mask


# ---- slots outside the format ----

FB_DIMS = (4096, 4096, 1, 32, 8, 512, 64)
TARGETS = {"wk": ("qkv", (2, 3)), "wo": ("wo", (0, 1)), "w2": ("ffn2", (0, 1)), "wcls": ("cls", (0, 1))}


@pytest.fixture(scope="module")
def fb_blob(ck):
    cfg = ck.Config(*FB_DIMS)
    rng = np.random.default_rng(5)
    blob = np.empty(ck.weights_count(cfg, False), np.float32)
    for x in ck.tensor_table(cfg, False):
        blob[x.offset:x.offset + x.count] = x.bias + x.scale * rng.uniform(-1, 1, x.count).astype(np.float32)
    return cfg, blob


@pytest.mark.parametrize("plant", ("span_31", "nan"))
@pytest.mark.parametrize("target", list(TARGETS))
def test_a_slot_outside_the_format_takes_only_its_own_launch_back_to_f32(gpu, ck, fb_blob, target, plant):
    cfg, blob = fb_blob
    x = {t.name: t for t in ck.tensor_table(cfg, False)}[target]
    m = blob[x.offset:x.offset + x.count]
    at, keep = 5 * x.shape[-1] + 7, None
    keep = m[at]
    e_max = int(((m.view(np.uint32) >> 23) & 0xFF).max())
    m[at] = np.float32(np.nan) if plant == "nan" else np.float32(2.0) ** (e_max - 31 - 127)
    try:
        w = gpu.Weights(cfg, blob, False)
    finally:
        m[at] = keep
    try:
        kind, left = TARGETS[target]
        for k in KINDS:
            full = (3, 3) if k == "qkv" else (1, 1)
            assert count_kind(gpu, w, k) == (left if k == kind else full), k
        assert count_w13(gpu, w) == (1, 1)
        ref_logits, ref_toks = decode(runstate(gpu, cfg, packed_w=0), w)
        logits, toks = decode(runstate(gpu, cfg), w)
        assert np.array_equal(logits, ref_logits)
        assert np.array_equal(toks, ref_toks)
    finally:
        w.close()
