"""The inputs the tests of the batched step and the verify pass on int8 group-quantized weights share (DESIGN.md 4.25;
tests/test_gpu_q8_batch.py on the GPU, tests/test_q8_batch_cpu.py checks on the CPU what that file relies on).

Reference runs are tests/q8_prefill_cases.py's token runs and references, unchanged ("64": 32 tokens, "512": 24, "288" and
"tall": 12): on them the two CPU modes of tests/ref_q8.py agree at the parity bar at every position.

Two more shapes are held by EXACT relations only (bit for bit between two device runs), so any seed serves:
  "kv24"    (96, 256, 2, 4, 1, 260, 160, 32): head_size 24; kv_dim 24 -- a K / V segment of one and a half row tiles of 16,
            behind six tiles of q; a vocabulary that is a multiple of 4 and not of 16; 160 positions: three verify segments
            of 64; dim of three groups and hidden_dim of eight, so some waves of the product get no group at all.
  "wide80"  tests/q8_prefill_long_cases.py's: head size 80, group size 64, 640 positions.
Shapes are (dim, hidden_dim, layers, heads, kv heads, vocab, seq_len, group size), as in tests/q8_cases.py.
"""
import functools

import numpy as np

import q8_cases
import q8_prefill_cases as pc
import q8_prefill_long_cases as lc

f32 = np.float32
BATCH_MAX = 16
SEG = 64          # csrc/batch_decode.h kVerifySeg
TILE = 16         # csrc/q8_gemm_device.h: weight rows, and token rows, of a tile
KV24 = (96, 256, 2, 4, 1, 260, 160, 32)
KV24_SEED = 5
EXACT_SHAPES = ("64", "kv24", "wide80")

# c. draft invariance: (shape, pos0, rows)
VERIFY_CASES = [(name, 0, n) for name in ("64", "kv24") for n in (2, 8, 16)] + \
               [("kv24", 60, n) for n in (2, 8, 16)] + [("wide80", 130, n) for n in (2, 8, 16)]
# d. the reference runs: shape -> the verify calls' row counts (consecutive from position 0)
REFERENCE_CALLS = {"64": [16, 16], "512": [16, 8], "288": [12], "tall": [12]}
BATCH_REF_STEPS = 12


@functools.lru_cache(maxsize=None)
def _kv24():
    import __graft_entry__ as ge
    ck = ge.load_package().checkpoint
    cfg = ck.Config(*KV24[:7])
    blob = ck.synth_blob(cfg, True, KV24_SEED)
    return cfg, KV24[7], blob, ck.v2_body_from_f32(cfg, blob, True, KV24[7])


def shape(name):
    return KV24 if name == "kv24" else lc.SHAPES[name] if name in lc.SHAPES else q8_cases.SHAPES[name]


def model(name):
    """(cfg, gs, the f32 blob, the version-2 body quantized from it); shared classifier."""
    if name == "kv24":
        return _kv24()
    return lc.model(name) if name in lc.SHAPES else q8_cases.model(name)


def tokens(name, n=None):
    """The shape's token run: q8_prefill_cases' for the reference shapes, a seeded draw of seq_len ids for the others."""
    if name in pc.RUN_LENGTH:
        t = pc.tokens(name)
    elif name in lc.SHAPES:
        t = lc.tokens(name, lc.SHAPES[name][6])
    else:
        t = np.random.default_rng(1000 + KV24_SEED).integers(2, KV24[5], KV24[6]).astype(np.int32)
    return t if n is None else t[:n]


def batch_feeds(name):
    """[3, BATCH_REF_STEPS]: what the three sequences of the batched reference run are fed -- the shape's run, the run
    reversed, the run rotated by five."""
    t = tokens(name, BATCH_REF_STEPS)
    return np.stack([t, t[::-1], np.roll(t, 5)]).astype(np.int32)


def embedding_rows(emb_q, emb_s, toks, gs):
    """Rows toks of a quantized table as the device forms them: f32(q) * s, one f32 rounding an element."""
    q = emb_q[toks].astype(f32)
    return (q.reshape(len(toks), -1, gs) * emb_s[toks][:, :, None]).astype(f32).reshape(len(toks), -1)


def qkv_tiles(name):
    """The q | k | v launch's blocks restated: (tiles of q, tiles of k or v, live rows of the last q tile, of the last k / v
    tile)."""
    dim, _, _, heads, kv_heads = shape(name)[:5]
    kvd = dim // heads * kv_heads
    return -(-dim // TILE), -(-kvd // TILE), dim - (-(-dim // TILE) - 1) * TILE, kvd - (-(-kvd // TILE) - 1) * TILE
