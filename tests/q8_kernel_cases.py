"""Inputs of the fused prologue's tight test (tests/test_gpu_q8_kernel.py, part d), built here so that
tests/test_ref_q8_cpu.py can check on the CPU what the GPU test relies on: the reference's integers are the only correct
ones.

x is integers k in [-16, 16] times 2^-3: every partial sum of squares is an integer multiple of 2^-6 below 2^24 of them, so
it is exact in f32 in any order (with or without fused multiply-adds) and the device's rms factor does not depend on its
reduction tree -- it is a few roundings of one exact number.  The rmsnorm weight is m / 8, m in 8 .. 15, so the normalised
value is s * (k m) / 64 and a quotient of the activation rule is 127 a / amax up to f32 noise, a = k m, amax the group's
largest |a|.  Such a quotient lies on a rounding boundary only where 254 a / amax is an odd integer: the fraction
a / amax in lowest terms then has denominator 2 or 254, 127 is prime and amax <= 240 is never a multiple of it, so
|a| = amax / 2 exactly is the only tie.  The builder moves such an element one step towards zero (which never makes a
new maximum); every other quotient is a multiple of 1 / amax away from an integer, at least 1 / (2 * 240) from a
boundary.  test_ref_q8_cpu.py asserts the margin of 2^-10 on the reference's own f32 quotients."""
import functools

import numpy as np

import ref_q8

f32 = np.float32
PROLOGUE_CASES = [(n, gs, norm) for n in (288, 4096, 11008) for gs in (32, 64) if n % gs == 0 for norm in (False, True)]
PROLOGUE_ROWS = 6
MARGIN = 2.0 ** -10


@functools.lru_cache(maxsize=None)
def prologue_case(n, gs, norm):
    """(x [n] f32, rms_w [n] f32 or None, wq [d, n], ws [d, n // gs]) of one case"""
    rng = np.random.default_rng(n * 5 + gs + (1000 if norm else 0))
    k = rng.integers(-16, 17, n)
    m = rng.integers(8, 16, n) if norm else np.ones(n, np.int64)
    kg, mg = k.reshape(-1, gs), m.reshape(-1, gs)   # (views: the repairs below change k)
    for g in range(kg.shape[0]):
        if not kg[g].any():
            kg[g, 0] = 5
        a = kg[g] * mg[g]
        half = 2 * np.abs(a) == np.abs(a).max()
        if norm:   # (without the norm the device's values are the input's own: a tie is the same tie on either side)
            kg[g][half] -= np.sign(kg[g][half])
    x = (k.astype(np.float64) * 0.125).astype(f32)
    rms_w = (m.astype(np.float64) / 8.0).astype(f32) if norm else None
    d = PROLOGUE_ROWS
    wq = rng.integers(-127, 128, (d, n)).astype(np.int8)
    ws = (rng.random((d, n // gs)) * 0.02 + 1e-4).astype(f32)
    for a in (x, wq, ws) + ((rms_w,) if norm else ()):
        a.setflags(write=False)
    return x, rms_w, wq, ws


@functools.lru_cache(maxsize=None)
def prologue_reference(n, gs, norm):
    """From those inputs in float64: (xq, xs) of the activation rule on the normalised values rounded to f32, the smallest
    distance of a quotient to a rounding boundary, and the product's terms [d, n // gs]."""
    x, rms_w, wq, ws = prologue_case(n, gs, norm)
    v = x.astype(np.float64)
    if norm:   # main.zig:432-468 in float64
        s = 1.0 / np.sqrt(np.sum(v * v) / n + 1e-5)
        v = (v * s) * rms_w.astype(np.float64)
    margins = []
    xq, xs = ref_q8.quantize_act(v.astype(f32), gs, margins)
    return xq, xs, margins[0], ref_q8.matvec_terms64(wq, ws, xq, xs, gs)
