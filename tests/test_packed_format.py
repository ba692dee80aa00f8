"""The 29-bit packed weight format (csrc/packed_w.h) without a GPU: a numpy statement of the encoder and
decoder round-trips every f32 bit pattern the format admits, the encodability rule takes +-0 and a span of exactly 30
binades and refuses a span of 31, a denormal, NaN and Inf; the chunk geometry gives 116 bytes per 128 of f32 at the 7B
widths; the L2Z_PACKED_W knob and the test-only calls are where the ABI says."""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "llama2.zig_amd", "csrc")


def lane_dw(s):
    return (29 * s + 3) // 4


def steps(n4, b, w):
    return sum(1 for k in range(4) if b * 1024 + 64 * w + 256 * k < n4)


def pair_dw(n4):
    nb = (n4 + 1023) // 1024
    return (nb - 1) * 4 * 64 * 29 + sum(64 * lane_dw(steps(n4, nb - 1, w)) for w in range(4))


def encodable(m):
    b = np.ascontiguousarray(m, np.float32).view(np.uint32).ravel()
    e = (b >> 23) & 0xFF
    if np.any(e == 255) or np.any((e == 0) & ((b & 0x7FFFFF) != 0)):
        return False
    nz = e[e != 0]
    return nz.size == 0 or int(nz.min()) + 30 >= int(nz.max())


def e_base(m):
    e = (np.ascontiguousarray(m, np.float32).view(np.uint32) >> 23) & 0xFF
    return int(e.max())


def encode_t(v, eb):
    v = np.uint32(v)
    e = (int(v) >> 23) & 0xFF
    c = 0 if e == 0 else e - (eb - 31)
    assert 0 <= c <= 31
    return (int(v) & 0x807FFFFF) | (c << 23)


def encode_lane(vals, eb):
    """vals: one lane's 8 S values (uint32) in (step, row, component) order -> lane_dw(S) dwords"""
    s = len(vals) // 8
    n, x = lane_dw(s), len(vals) - lane_dw(s)
    d = [encode_t(v, eb) for v in vals[:n]]
    for j in range(x):
        t = encode_t(vals[n + j], eb)
        p = ((t << 1) | (t >> 31)) & 0x1FFFFFFF
        for b in range(29):
            st = 29 * j + b
            d[st // 3] |= ((p >> b) & 1) << (28 + st % 3)
    return d


def decode_lane(d, s, eb):
    n, x = lane_dw(s), 8 * s - lane_dw(s)
    t = [w & 0x8FFFFFFF for w in d[:n]]
    for j in range(x):
        p = 0
        for b in range(29):
            st = 29 * j + b
            p |= ((d[st // 3] >> (28 + st % 3)) & 1) << b
        t.append(((p >> 1) | (p << 31)) & 0xFFFFFFFF)
    f = np.array(t, np.uint32).view(np.float32).astype(np.float32)
    return np.ldexp(f, eb - 31).astype(np.float32).view(np.uint32)  # exact: every result is normal or +-0


def random_matrix_values(rng, n, eb, span=30):
    e = rng.integers(eb - span, eb + 1, n)
    e[rng.random(n) < 0.1] = 0
    m = rng.integers(0, 1 << 23, n)
    m[e == 0] = 0
    s = rng.integers(0, 2, n)
    return ((s << 31) | (e << 23) | m).astype(np.uint32)


def test_lane_round_trip_is_bit_exact_for_every_step_count():
    rng = np.random.default_rng(1)
    for s in (1, 2, 3, 4):
        for eb in (31, 100, 127, 200, 254):
            for _ in range(200):
                v = random_matrix_values(rng, 8 * s, eb)
                v[0] = eb << 23  # the matrix maximum sits in this lane
                d = encode_lane([int(x) for x in v], eb)
                assert len(d) == lane_dw(s) and all(0 <= w < 1 << 32 for w in d)
                assert np.array_equal(decode_lane(d, s, eb), v), (s, eb)


def test_encodable_rule_edge_cases():
    base = np.array([0.5, -0.75, 0.25, 0.125], np.float32)
    eb = e_base(base)
    assert encodable(base)
    assert encodable(np.concatenate([base, np.float32([0.0, -0.0])]))              # +-0
    assert encodable(np.concatenate([base, [np.ldexp(np.float32(1), eb - 127 - 30)]]))  # span exactly 30
    assert not encodable(np.concatenate([base, [np.ldexp(np.float32(1), eb - 127 - 31)]]))  # span 31
    assert not encodable(np.concatenate([base, np.float32([1e-40])]))              # denormal
    assert not encodable(np.concatenate([base, np.float32([np.nan])]))
    assert not encodable(np.concatenate([base, np.float32([np.inf])]))
    assert not encodable(np.concatenate([base, np.float32([-np.inf])]))
    assert encodable(np.zeros(8, np.float32))                                       # all zeros: every code 0
    # the edge values that are encodable round-trip
    v = np.concatenate([base, np.float32([0.0, -0.0, np.ldexp(np.float32(-1.5), eb - 127 - 30), 0.3])]).view(np.uint32)
    assert np.array_equal(decode_lane(encode_lane([int(x) for x in v], eb), 1, eb), v)


def test_chunk_geometry_of_the_7b_widths():
    assert [lane_dw(s) for s in range(5)] == [0, 8, 15, 22, 29]
    assert pair_dw(1024) == 7424                       # n = 4096: 4 waves x 64 lanes x 29 dwords
    assert pair_dw(1024) * 4 / (2 * 4096 * 4) == 29 / 32
    assert [steps(2752, 2, w) for w in range(4)] == [3, 3, 3, 2]   # n = 11008: the partial last batch
    assert pair_dw(2752) == 20032
    assert pair_dw(2752) * 4 / (2 * 11008 * 4) < 0.91


def test_c_header_matches_the_numpy_statement():
    src = open(os.path.join(CSRC, "packed_w.h")).read()
    assert "(29 * s + 3) / 4" in src
    assert "0x807fffffu" in src and "0x8fffffffu" in src
    assert "min_e + 30 >= max_e" in src


def test_knob_and_test_calls_abi(B):
    tn = open(os.path.join(CSRC, "tunables.cpp")).read()
    assert re.search(r'env_int\("L2Z_PACKED_W", &t\.packed_w\)', tn)
    assert '{"L2Z_PACKED_W", &t.packed_w}' in tn
    assert re.search(r"int packed_w = 1;", open(os.path.join(CSRC, "tunables.h")).read())
    B.option_set("L2Z_PACKED_W", 0)   # settable in-process without a device (scripts/ab.py A/B)
    B.option_set("L2Z_PACKED_W", 1)
    for s in ("l2z_weights_packed_count", "l2z_weights_packed_read"):
        assert s in B.declared_symbols("test")
        assert s not in B.declared_symbols("product")
    assert "L2Z_PACKED_W" in open(os.path.join(ROOT, "DESIGN.md")).read()
