"""Hard checkpoints for the forward-pass families, and their float64 reference (DESIGN.md "Hard checkpoints").

`checkpoint.synth_blob` weights are uniform with variance 1 / dim: attention scores with a standard deviation near 1, a
softmax that is close to flat, no activation channel that stands out.  `hard_blob` edits such a blob into the statistics of
trained checkpoints -- peaked attention, exponentials that underflow to exactly 0, a few channels far larger than the rest
-- and `reference` gives, for ONE token chain per (shape, kind), the float64 logits of every position and a bar per row that
is derived from the reference's own fp32 readings alone:

    D[p]   = max over orc.ALL_MODES of max |z_mode[p] - z64[p]|       (how far an fp32 reading of the reference lies)
    bar[p] = LOGIT_ATOL + 4 * D[p]                                      (the factor of test_gpu_inside_reference_spread)

Nothing in it is taken from a GPU.  tests/test_hard_reference_cpu.py checks without a GPU that the regimes hold and that
the bar leaves (almost) no row out of the token comparison; tests/test_gpu_hard_parity.py runs the families against it.
"""
import functools
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ref_numpy import NumpyModel
from test_gpu_parity import LOGIT_ATOL

FACTOR = 4          # tests/test_gpu_parity.py test_gpu_inside_reference_spread
SEED = 23
KINDS = ("flat", "peaked", "onehot", "outlier")
WIDE = dict(dim=512, hidden_dim=1408, n_layers=2, n_kv_heads=2, vocab_size=1024, seq_len=192)
SHAPES = {
    # tests/test_gpu_wide_decode.py's kvmul3: head size 48, one part of 3 query heads in an attention block made for 4
    "kvmul3": dict(dim=288, hidden_dim=768, n_layers=2, n_heads=6, n_kv_heads=2, vocab_size=1024, seq_len=160),
    "hs64h": dict(WIDE, n_heads=8),    # head size 64, kv_mul 4
    "hs128h": dict(WIDE, n_heads=4),   # head size 128, kv_mul 2
}
CASES = [("kvmul3", "flat"), ("kvmul3", "peaked"), ("kvmul3", "onehot"), ("kvmul3", "outlier"),
         ("hs64h", "onehot"), ("hs64h", "flat"), ("hs128h", "peaked"), ("hs128h", "outlier")]
CASE_IDS = [f"{s}-{k}" for s, k in CASES]
EDGES = (0, 63, 64, 65, 127, 128)   # after seq_len - 1: the depths every list of depths starts with
THREADS = 8                         # the reference's passes side by side
EXP_ZERO = 104.0                    # f32 expf(-x) is exactly 0 from here on (below the smallest subnormal, 2^-149)


def config(ck, shape):
    return ck.Config(**SHAPES[shape])


def hard_blob(ck, cfg, seed, kind):
    """synth_blob(cfg, unshared, seed) with its statistics edited in place through carve()'s views"""
    blob = ck.synth_blob(cfg, False, seed)
    w = ck.carve(cfg, blob, False)
    if kind == "flat":        # every score exactly 0, every softmax weight exactly 1 / (pos + 1)
        w["wq"][...] = 0.0
    elif kind == "peaked":    # score spreads of tens
        w["wq"] *= np.float32(8)
    elif kind == "onehot":    # spreads past the point where expf underflows to 0
        w["wq"] *= np.float32(32)
    elif kind == "outlier":   # four channels tens of times larger than the rest, under a peaked attention
        w["wq"] *= np.float32(4)
        ch = np.random.default_rng([seed, 77]).choice(cfg.dim, 4, replace=False)
        w["rms_att_weight"][:, ch] *= np.float32(16)
        w["rms_ffn_weight"][:, ch] *= np.float32(16)
        w["token_embedding_table"][:, ch] *= np.float32(8)
    else:
        raise ValueError(kind)
    return blob


def chain(cfg):
    """the case's token chain T: BOS, then seq_len - 1 drawn tokens"""
    return np.array([1] + np.random.default_rng([SEED, 5]).integers(2, cfg.vocab_size, cfg.seq_len - 1).tolist(), np.int32)


def readings(orc, cfg, blob, T):
    """{mode: logits [len(T), vocab]} of the oracle's 12 readings of the reference for one model"""
    return {mode: r[0] for mode, r in readings_of(orc, [(cfg, blob, T)]).items()}


def readings_of(orc, models):
    """{mode: [logits [len(T), vocab] per (cfg, blob, T) of models]}.  The oracle's mode is process-global, so the modes run
    one after another -- with the models of one mode side by side, on threads (the oracle's calls release the GIL and read
    the mode only) -- and the default is put back."""
    def run(model):
        cfg, blob, T = model
        m = orc.Model(cfg.as_i32(), blob, False)
        z = np.stack([m.transformer(int(t), p) for p, t in enumerate(T)])
        m.close()
        return z
    out = {}
    try:
        with ThreadPoolExecutor(min(len(models), THREADS)) as ex:
            for mode in orc.ALL_MODES:
                orc.set_mode(*mode)
                out[mode] = list(ex.map(run, models))
    finally:
        orc.set_mode(8, False, False)
    return out


def spread_of(z64, runs):
    """D[p]: the largest distance of a reading from the float64 logits, per position"""
    return np.max([np.abs(r.astype(np.float64) - z64).max(axis=1) for r in runs.values()], axis=0)


def float64_pass(ck, cfg, blob, T):
    """(z64, spread, uniform) of NumpyModel over the chain, through its probe"""
    spread = np.zeros((cfg.n_layers, cfg.n_heads, len(T)))
    uniform = np.zeros((cfg.n_layers, cfg.n_heads, len(T)), bool)

    def probe(l, h, pos, s, att):
        spread[l, h, pos] = s
        uniform[l, h, pos] = bool(np.all(att == 1.0 / (pos + 1)))
    nm = NumpyModel(ck, cfg, blob, False, probe=probe)
    return np.stack([nm.transformer(int(t), p) for p, t in enumerate(T)]), spread, uniform


@functools.lru_cache(maxsize=None)
def references(ck, orc):
    """{(shape, kind): reference} of all CASES, computed together (see readings_of) once per process"""
    models = []
    for shape, kind in CASES:
        cfg = config(ck, shape)
        models.append((cfg, hard_blob(ck, cfg, SEED, kind), chain(cfg)))
    with ThreadPoolExecutor(THREADS) as ex:   # the float64 passes beside the oracle's
        f64 = [ex.submit(float64_pass, ck, *m) for m in models]
        runs = readings_of(orc, models)
        f64 = [f.result() for f in f64]
    out = {}
    for i, (shape, kind) in enumerate(CASES):
        cfg, blob, T = models[i]
        z64, spread, uniform = f64[i]
        D = spread_of(z64, {mode: r[i] for mode, r in runs.items()})
        two = np.partition(z64, -2, axis=1)[:, -2:]
        r = types.SimpleNamespace(shape=shape, kind=kind, cfg=cfg, blob=blob, T=T, z64=z64, z_default=runs[(8, 0, 0)][i], D=D,
                                  bar=LOGIT_ATOL + FACTOR * D, top=np.argmax(z64, axis=1), margin=two[:, 1] - two[:, 0],
                                  spread=spread, uniform=uniform)
        for a in vars(r).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[(shape, kind)] = r
    return out


def reference(ck, orc, shape, kind):
    """The case's reference, never changed after it is made (its arrays are read-only): cfg, blob, T; z64 [L, vocab] the
    float64 logits of every chain position; z_default the default oracle reading; D, bar, top, margin per position; spread
    [layer, head, pos] the float64 score spread of every softmax and uniform [layer, head, pos] whether its weights all
    equal 1 / (pos + 1) exactly."""
    return references(ck, orc)[(shape, kind)]


def log_softmax64(z):
    z = np.asarray(z, np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))
