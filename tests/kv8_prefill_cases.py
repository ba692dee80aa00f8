"""What the tests of the prompt pass into int8 KV rows share (tests/test_gpu_kv8_prefill.py,
tests/test_kv8_prefill_reference_cpu.py): a shape with head_size 64 and GQA -- the smallest that takes the matrix-core
attention -- and its float64 reference with int8 rows, teacher-forced over N_REF tokens.

SEED is the first of seeds 0 .. 39 for which the reference's own f32 and f64 modes have no position over the parity bar
(a flipped byte stays in the cache and moves every later position) UNDER EVERY KERNEL SET numpy may dispatch to: its f32 exp,
cos and sin differ in the last bit between the AVX-512 kernels, the AVX2 ones and the baseline, and that bit decides which
side of a rounding boundary a byte lands on.  Positions over the bar, with AVX-512 / without (measured on the CPU, the second
by NPY_DISABLE_CPU_FEATURES): seed 0 49 / 77, seed 1 none / 50 (up to 1.8e-2 of the scale), seed 2 none / none, also with AVX2
and FMA3, and with AVX, disabled: largest deviation between the modes 3.9e-7 / 3.3e-7 of the scale;
tests/test_kv8_prefill_reference_cpu.py asserts it on the kernels of the machine it runs on.
"""
import functools

import numpy as np

import kv8_cases
import ref_q8

SHAPE = (128, 384, 2, 2, 1, 512, 160, 64)   # dim, hidden_dim, layers, heads, kv heads, vocab, seq_len, group size
SEED = 2
N_REF = 101


@functools.lru_cache(maxsize=None)
def model(seed=SEED):
    """(cfg, gs, the version-2 body); shared classifier"""
    import __graft_entry__ as ge
    ck = ge.load_package().checkpoint
    cfg = ck.Config(*SHAPE[:7])
    return cfg, SHAPE[7], ck.v2_body_from_f32(cfg, ck.synth_blob(cfg, True, seed), True, SHAPE[7])


def tokens(seed=SEED):
    return np.random.default_rng(1000 + seed).integers(2, SHAPE[5], N_REF).astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(mode="f64", seed=SEED):
    """(logits [N_REF, V], dequantized K rows [L, N_REF, kvd], V rows) of tokens()[p] at position p"""
    import __graft_entry__ as ge
    ck = ge.load_package().checkpoint
    cfg, gs, body = model(seed)
    m = ref_q8.Q8Model(cfg, ck.v2_carve(cfg, body, True, gs), gs, mode)
    m.kc, m.vc = (kv8_cases.Kv8Rows(m.kc.shape, cfg.head_size, m.ft) for _ in range(2))
    z = np.stack([m.transformer(int(t), p) for p, t in enumerate(tokens(seed))])
    return z, m.kc.a[:, :N_REF].copy(), m.vc.a[:, :N_REF].copy()
