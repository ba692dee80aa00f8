"""The inputs the long-prompt tests of the batched prompt pass on int8 group-quantized weights share (DESIGN.md 4.24;
tests/test_gpu_q8_prefill_long.py on the GPU, tests/test_q8_prefill_long_cpu.py checks on the CPU what that file relies on):
the GEMM cases past one column of blocks with the launcher's grid arithmetic restated (their operands are
tests/test_gpu_q8_prefill.py's gemm_inputs), two checkpoints with seq_len 640, their token runs and the chunk plans the
whole-pass tests set.

Shapes are (dim, hidden_dim, layers, heads, kv heads, vocab, seq_len, group size), as in tests/q8_cases.py.  Both keep
the prompt attention on its block-per-(head, query) kernel at every chunk length used (attention_form below restates the
launcher's choice), whose result for a query depends on pos0 + its index alone; with the GEMM's row identity the whole
pass is then the same bits however the prompt is cut into chunks and calls.

The reference run ("long64", 300 tokens).  The pass is discontinuous, so the seed is the one of seeds 0 .. 299 with the
largest distance of any activation quotient to a rounding boundary among those on which the two modes of tests/ref_q8.py
agree at the parity bar at all 300 positions (scripts/q8_long_seed_sweep.py; SWEEP holds what it printed).
"""
import functools

import numpy as np

f32 = np.float32
TILE, NT_MAX = 16, 8   # q8_gemm.hip: a token tile, and the most token tiles a block takes

# ---------------------------------------------------------------- the GEMM past one column of blocks
# (m, d, n, gs) -> (columns of blocks, token tiles of the last column) each case was built for
GEMM_LONG_CASES = {
    (129, 36, 288, 32): (2, 1),      # a second column holding one tile with one live row; a row tile that is not full
    (144, 100, 768, 64): (2, 1),     # nine tiles exactly
    (256, 288, 768, 64): (2, 8),     # two full columns
    (257, 4, 4224, 64): (3, 1),      # one row into a third column
    (300, 100, 11008, 32): (3, 3),   # columns of 8, 8 and 3 tiles; 344 groups: eleven K batches a wave
    (300, 2816, 288, 32): (3, 3),    # 176 row tiles by 3 columns
    (1024, 36, 4096, 64): (8, 8),    # the default chunk cap: eight full columns
    (2048, 4, 64, 64): (16, 8),      # the largest L2Z_PF_CHUNK; one group, so seven idle waves
}


def gemm_grid(m, d):
    """launch_q8_gemm's arithmetic: (token tiles, tiles a block NT, columns of blocks n_tt, tiles of the last column, row
    tiles, live rows of the last token tile)."""
    n_tiles = -(-m // TILE)
    nt = 1 if n_tiles <= 1 else 2 if n_tiles <= 2 else 4 if n_tiles <= 4 else NT_MAX
    n_tt = -(-n_tiles // nt)
    return n_tiles, nt, n_tt, n_tiles - (n_tt - 1) * nt, -(-d // 16), m - (n_tiles - 1) * TILE


def row_slices(m):
    """The calls of at most 16 rows the row identity compares with: [16 i, 16 i + 16)."""
    return [slice(i, min(i + TILE, m)) for i in range(0, m, TILE)]


# ---------------------------------------------------------------- the whole pass on long prompts
SHAPES = {
    "long64": (64, 192, 2, 4, 2, 512, 640, 32),
    "wide80": (320, 832, 2, 4, 2, 512, 640, 64),   # head size 80, 13 groups in hidden_dim, GQA
}
SEEDS = {"long64": 208, "wide80": 7}   # "long64": see SWEEP; "wide80" is held by exact relations only, any seed serves
# the sweep's print: 76 of seeds 0 .. 299 agree at every position; margins (the smaller of the two modes', of a step): 9.06e-6
# (seed 208), 7.63e-6 (seeds 214 and 67), 5.72e-6 (seeds 89 and 0); about 1 s a seed and mode
SWEEP = {"seeds": 300, "tokens": 300, "agreeing": 76, "best": 208, "margin": 9.06e-6}
REF_TOKENS = 300
REF_LOGIT_POSITIONS = (127, 128, 143, 255, 256, 299)

# (shape-independent) the chunk plans of tests a, b, c and e: (L2Z_PF_CHUNK, the tokens of each call)
CHUNK_PLANS = {
    "a one chunk": (2048, [300]),
    "a calls of 128": (2048, [128, 128, 44]),
    "b 144 in one call": (144, [300]),
    "b 144 as calls": (144, [144, 144, 12]),
    "b 48 in one call": (48, [100]),
    "b 48 as calls": (48, [48, 48, 4]),
    "c grow": (2048, [20, 600, 20]),
    "d reference": (2048, [300]),
    "e generate": (2048, [140]),
    "e generate as calls": (2048, [128, 12]),
}


def chunks_of(chunk, n_tokens):
    """The chunk lengths one call of n_tokens takes with L2Z_PF_CHUNK = chunk (tunables.cpp's prefill_next_chunk with the
    knob set: the knob's length while that many remain, then the rest)."""
    chunk = min(max(chunk, 16), 2048)
    out = []
    while n_tokens > 0:
        out.append(min(chunk, n_tokens))
        n_tokens -= out[-1]
    return out


def attention_form(n_heads, head_size, P):
    """launch_prefill_attention's choice restated for aligned f32 rows (form 0: by shape): "flash", "tiled" or "query"
    (a block per (head, query))."""
    q_tiles = (P + 63) // 64
    if n_heads * q_tiles >= 32 and P > 32 and head_size in (64, 128):
        return "flash"
    lds_t = (3 * 64 * (head_size + 1) + 64 * 65 + 3 * 64) * 4
    if n_heads * q_tiles >= 128 and lds_t <= 160 * 1024 and (head_size + 31) // 32 <= 8 and head_size % 4 == 0:
        return "tiled"
    return "query"


def config(ck, name):
    return ck.Config(*SHAPES[name][:7]), SHAPES[name][7]


@functools.lru_cache(maxsize=None)
def _model(name, seed, gs):
    import __graft_entry__ as ge
    ck = ge.load_package().checkpoint
    cfg = ck.Config(*SHAPES[name][:7])
    blob = ck.synth_blob(cfg, True, seed)
    return cfg, gs, blob, ck.v2_body_from_f32(cfg, blob, True, gs)


def model(name, seed=None, gs=None):
    """(cfg, gs, the f32 blob, the version-2 body quantized from it at gs); shared classifier."""
    return _model(name, SEEDS[name] if seed is None else seed, SHAPES[name][7] if gs is None else gs)


def tokens(name, n, seed=None):
    """The first n of the shape's 640 tokens."""
    V, S = SHAPES[name][5], SHAPES[name][6]
    rng = np.random.default_rng(1000 + (SEEDS[name] if seed is None else seed))
    return rng.integers(2, V, S).astype(np.int32)[:n]


@functools.lru_cache(maxsize=None)
def reference(mode="f64", seed=None):
    """(logits [300, V], K rows [L, 300, kvd], V rows, the smallest distance of an activation quotient to a rounding
    boundary) of "long64" on its first 300 tokens, computed once; read-only."""
    import __graft_entry__ as ge
    import ref_q8
    ck = ge.load_package().checkpoint
    cfg, gs, _, body = model("long64", seed)
    toks = tokens("long64", REF_TOKENS, seed)
    z, m = ref_q8.run_positions(ck, cfg, body, True, gs, toks, mode)
    out = (z, m.kc[:, :REF_TOKENS].copy(), m.vc[:, :REF_TOKENS].copy())
    for a in out:
        a.setflags(write=False)
    return out + (min(m.margins),)
