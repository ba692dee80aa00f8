"""The 28-bit packed form on the device (csrc/packed_w.h pk28), on one-layer models whose every kind of
row launch is 4096 wide (W2 included), and on one with an 11008-wide W2 that must stay at 29 bits:

  * a numpy uniform blob has natural escapes: every slot reports 28 bits and decodes on the device to the f32 bits;
  * the CPU test's escape placements (tests/test_packed28_format.py PLANTS: eight, at the corners of the position space)
    planted into one pair of each of Wq, Wo, W1, W2 and the classifier: the read-back is equal, and the stepped pass's
    logits over 16 positions are bit-identical among L2Z_PACKED_BITS=28, =29 and L2Z_PACKED_W=0, as are the 16 greedy tokens;
  * nine escapes in one pair of Wk, Wo, W2 or the classifier alone: that kind (q|k|v: all three slots) reports 29, the
    others 28, and the results are those of the f32 pass;
  * the 11008-wide W2 reports 29 whatever the knob says, and with L2Z_PACKED_BITS=29 no slot reports 28;
  * the default mask of kinds (L2Z_PACKED28_KINDS: ffn13 and the classifier) leaves the other kinds at 29, same results.

Every other case allows every kind the 28-bit form (L2Z_PACKED28_KINDS=-1).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_packed_kinds import FB_DIMS, KINDS, decode, f32_slots, read_kind, runstate
from test_packed28_format import INSIDE, MAX_ESC, PLANTS, escapes, plant_bits, row_col

pytestmark = pytest.mark.gpu

DEFAULT_BITS = 28            # csrc/tunables.h packed_bits
DEFAULT_KINDS28 = 40         # ... packed28_kinds: ffn13 | cls, the kinds the 28-bit form made faster at 7B
SLOTS = [(k, j) for k in KINDS for j in range(3 if k == "qkv" else 1)]
PAIR = 3                     # the pair the escapes are planted into
W2_WIDE_DIMS = (4096, 11008, 1, 32, 8, 512, 64)


def bits_kind(B, w, kind, slot=0):
    L = B.lib()
    L.l2z_weights_packed_bits_kind.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    b = C.c_int(-1)
    assert L.l2z_weights_packed_bits_kind(w.h, B.KINDS.index(kind), 0, slot, C.byref(b)) == 0
    return b.value


def all_bits(B, w):
    return {(k, j): bits_kind(B, w, k, j) for k, j in SLOTS}


def weights(B, cfg, blob, bits, seed=None, kinds28=-1):
    """a weights object packed at `bits`, every kind allowed the 28-bit form (the default mask keeps q|k|v and Wo at 29)"""
    B.option_set("L2Z_PACKED_BITS", bits)
    B.option_set("L2Z_PACKED28_KINDS", kinds28)
    try:
        return B.Weights(cfg, blob, False, seed=seed)
    finally:
        B.option_set("L2Z_PACKED_BITS", DEFAULT_BITS)
        B.option_set("L2Z_PACKED28_KINDS", DEFAULT_KINDS28)


def tensors(ck, cfg, blob):
    return {t.name: blob[t.offset:t.offset + t.count].reshape(-1, t.shape[-1]).view(np.uint32) for t in ck.tensor_table(cfg, False)}


def pair_rows(t, name, q):
    """the two rows (uint32 views) of pair q of the slot tensor `name` lies in, and the slot's base exponent"""
    if name == "w1":   # the W1 | W3 slot: pair q is W1's row q and W3's row q
        rows, mats = (t["w1"][q], t["w3"][q]), (t["w1"], t["w3"])
    else:
        rows, mats = (t[name][2 * q], t[name][2 * q + 1]), (t[name],)
    return rows, max(int(((m >> 23) & 0xFF).max()) for m in mats)


def plant_pair(t, name, n_escapes, q=PAIR):
    """exactly n_escapes escapes in pair q: its natural ones taken out, PLANTS[:n_escapes] and INSIDE written in"""
    rows, eb = pair_rows(t, name, q)
    for r in rows:
        r[escapes(r, eb)] = eb << 23
    for w, lane, i, off, sign in PLANTS[:n_escapes] + INSIDE:
        r, c = row_col(w, lane, i)
        rows[r][c] = plant_bits(eb, off, sign)
    assert sum(int(escapes(r, eb).sum()) for r in rows) == n_escapes


def max_escapes_per_pair(t, name):
    if name == "w1":
        eb = pair_rows(t, "w1", 0)[1]
        return int((escapes(t["w1"], eb).sum(axis=1) + escapes(t["w3"], eb).sum(axis=1)).max())
    eb = pair_rows(t, name, 0)[1]
    return int(escapes(t[name], eb).sum(axis=1).reshape(-1, 2).sum(axis=1).max())


@pytest.fixture(scope="module")
def base(ck):
    cfg = ck.Config(*FB_DIMS)
    rng = np.random.default_rng(5)
    blob = np.empty(ck.weights_count(cfg, False), np.float32)
    for x in ck.tensor_table(cfg, False):
        blob[x.offset:x.offset + x.count] = x.bias + x.scale * rng.uniform(-1, 1, x.count).astype(np.float32)
    return cfg, blob


def check_read_back(gpu, ck, cfg, w):
    for (kind, slot), m in f32_slots(ck, cfg, False, w).items():
        rc, got = read_kind(gpu, w, kind, 0, slot, *m.shape)
        assert rc == 0, (kind, slot)
        assert np.array_equal(got.view(np.uint32), m.view(np.uint32)), (kind, slot)


def test_natural_escapes_every_slot_at_28_bits_decodes_to_the_f32_bits(gpu, ck, base):
    cfg, blob = base
    t = tensors(ck, cfg, blob)
    for name in ("wq", "wk", "wv", "wo", "w1", "w2", "wcls"):
        worst = max_escapes_per_pair(t, name)
        assert 1 <= worst <= MAX_ESC, (name, worst)   # the blob has escapes, and no pair more than a record holds
    w = weights(gpu, cfg, blob, 28)
    try:
        assert all_bits(gpu, w) == {s: 28 for s in SLOTS}
        check_read_back(gpu, ck, cfg, w)
    finally:
        w.close()


def test_planted_record_same_bits_at_28_at_29_and_from_f32(gpu, ck, base):
    cfg, blob = base[0], base[1].copy()
    t = tensors(ck, cfg, blob)
    for name in ("wq", "wo", "w1", "w2", "wcls"):
        plant_pair(t, name, MAX_ESC)
    w28, w29 = weights(gpu, cfg, blob, 28), weights(gpu, cfg, blob, 29)
    try:
        assert all_bits(gpu, w28) == {s: 28 for s in SLOTS}
        assert all_bits(gpu, w29) == {s: 29 for s in SLOTS}
        check_read_back(gpu, ck, cfg, w28)
        check_read_back(gpu, ck, cfg, w29)
        ref_logits, ref_toks = decode(runstate(gpu, cfg, packed_w=0), w28)
        for w in (w28, w29):
            logits, toks = decode(runstate(gpu, cfg), w)
            assert np.array_equal(logits, ref_logits)
            assert np.array_equal(toks, ref_toks)
    finally:
        w28.close()
        w29.close()


OVERFLOW = {"wk": "qkv", "wo": "wo", "w2": "ffn2", "wcls": "cls"}


@pytest.mark.parametrize("target", list(OVERFLOW))
def test_nine_escapes_in_one_pair_keep_that_kind_at_29_bits(gpu, ck, base, target):
    cfg, blob = base[0], base[1].copy()
    plant_pair(tensors(ck, cfg, blob), target, MAX_ESC + 1)
    w = weights(gpu, cfg, blob, 28)
    try:
        assert all_bits(gpu, w) == {(k, j): 29 if k == OVERFLOW[target] else 28 for k, j in SLOTS}
        check_read_back(gpu, ck, cfg, w)
        ref_logits, ref_toks = decode(runstate(gpu, cfg, packed_w=0), w)
        logits, toks = decode(runstate(gpu, cfg), w)
        assert np.array_equal(logits, ref_logits)
        assert np.array_equal(toks, ref_toks)
    finally:
        w.close()


@pytest.mark.parametrize("bits", (28, 29))
def test_other_widths_stay_at_29_bits_and_the_knob_at_29_packs_nothing_at_28(gpu, ck, bits):
    cfg = ck.Config(*W2_WIDE_DIMS)
    w = weights(gpu, cfg, None, bits, seed=11)
    try:
        assert all_bits(gpu, w) == {(k, j): 29 if k == "ffn2" else bits for k, j in SLOTS}
        check_read_back(gpu, ck, cfg, w)
        ref_logits, ref_toks = decode(runstate(gpu, cfg, packed_w=0), w)
        logits, toks = decode(runstate(gpu, cfg), w)
        assert np.array_equal(logits, ref_logits)
        assert np.array_equal(toks, ref_toks)
    finally:
        w.close()


def test_default_mask_packs_ffn13_and_the_classifier_at_28_bits_only(gpu, ck, base):
    cfg, blob = base
    w = weights(gpu, cfg, blob, DEFAULT_BITS, kinds28=DEFAULT_KINDS28)
    try:
        assert all_bits(gpu, w) == {(k, j): 28 if k in ("ffn13", "cls") else 29 for k, j in SLOTS}
        check_read_back(gpu, ck, cfg, w)
        ref_logits, ref_toks = decode(runstate(gpu, cfg, packed_w=0), w)
        logits, toks = decode(runstate(gpu, cfg), w)
        assert np.array_equal(logits, ref_logits)
        assert np.array_equal(toks, ref_toks)
    finally:
        w.close()
