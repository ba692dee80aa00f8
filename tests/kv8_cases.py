"""What the tests of the int8 KV cache share (tests/test_gpu_kv8.py, tests/test_kv8_reference_cpu.py): the
reference of the wide q8 step on such a cache -- tests/ref_q8.py's pass with the K / V rows stored through the format's
rule -- and the checkpoints it is held against.

The shapes are tests/q8_cases.py's with its seeds, except "512": a flipped byte stays in the cache and moves every later
position, and with seed 121 the reference's own f32 and f64 modes disagree at positions 4, 10 and 11 (1.6e-2 of the scale).
SEED_512 is the first of seeds 0 .. 99 for which the two modes have no position over the parity bar.  Largest deviation
between the modes, as a fraction of the scale (measured on the CPU; tests/test_kv8_reference_cpu.py asserts the condition):
  "64" 2.6e-7   "288" 5.2e-7   "tall" 3.9e-7   "512" (seed SEED_512) 4.9e-7
"""
import functools

import numpy as np

import q8_cases
import ref_q8

f32 = np.float32
SEED_512 = 0
SEEDS = dict(q8_cases.SEEDS, **{"512": SEED_512})
SHAPES = tuple(q8_cases.SHAPES)


class Kv8Rows:
    """[layers, seq_len, kv_dim] rows that come back as the int8 cache gives them: a stored row is quantized a head slice
    at a time by the activation rule (of its f32 rounding) and read as f32(q) * s."""

    def __init__(self, shape, head_size, ft):
        self.a, self.hs = np.zeros(shape, ft), head_size

    def __setitem__(self, at, row):
        q, s = ref_q8.quantize_act(np.asarray(row).astype(f32), self.hs)
        self.a[at] = q.astype(f32) * np.repeat(s, self.hs)

    def __getitem__(self, at):
        return self.a[at]


def model(name):
    return q8_cases.model(name, SEEDS[name])


def tokens(name):
    return q8_cases.tokens(name, SEEDS[name])


def kv8_model(name, mode, seed=None):
    import __graft_entry__ as ge
    ck = ge.load_package().checkpoint
    cfg, gs, _, body = q8_cases.model(name, SEEDS[name] if seed is None else seed)
    m = ref_q8.Q8Model(cfg, ck.v2_carve(cfg, body, True, gs), gs, mode)
    m.kc, m.vc = (Kv8Rows(m.kc.shape, cfg.head_size, m.ft) for _ in range(2))
    return m


@functools.lru_cache(maxsize=None)
def reference(name, mode="f64", seed=None):
    """(logits [12, V], dequantized K rows [L, 12, kvd], V rows) of the shape's tokens at positions 0 .. 11"""
    m = kv8_model(name, mode, seed)
    toks = q8_cases.tokens(name, SEEDS[name] if seed is None else seed)
    z = np.stack([m.transformer(int(t), p) for p, t in enumerate(toks)])
    return z, m.kc.a[:, :q8_cases.N_POS].copy(), m.vc.a[:, :q8_cases.N_POS].copy()
