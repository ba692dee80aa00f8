"""The 28-bit packed weight form (csrc/packed_w.h namespace pk28) without a GPU: the header compiled
into a stand-alone host program under AddressSanitizer and UBSan, against a numpy statement of the same format.

  * round trip: 500 random lanes for each of several bases E, exponents E - 14 .. E and +-0, no escape among them;
  * geometry: a pair is 28672 bytes and the plane offsets of a wave's chunk cover each of its dwords once;
  * record building: pairs with 0, 1, 8 and 9 escapes at the corners of the position space (PLANTS): stream and record are
    the numpy statement's, stream plus record give back all 8192 values' bits, 9 escapes report overflow.
"""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "llama2.zig_amd", "csrc")

LANE_DW, CHUNK_DW, PAIR_DW, REC_DW, MAX_ESC, NO_ESC = 28, 64 * 28, 4 * 64 * 28, 16, 8, 0xFFFFFFFF

# (wave, lane, i, exponent - E, sign): the escapes planted into a pair, in the order the cases take them (not pos order).
# Waves 0 and 3, lanes 0 and 63, i = 0 and 27 (stored in place) and 28 and 31 (in the bit stream), the first exponent
# outside the window (E - 15) and the last the format admits (E - 30), both signs; the ninth overflows the record
PLANTS = [(3, 63, 31, -15, 1), (0, 0, 0, -15, 0), (0, 0, 27, -30, 1), (0, 63, 28, -15, 1), (3, 0, 31, -30, 0),
          (3, 63, 0, -15, 1), (3, 63, 27, -15, 0), (3, 63, 28, -30, 0), (1, 17, 13, -22, 0)]
# values that must NOT become escapes: the last exponent inside the window (E - 14), both signs, in place and in the bit
# stream, and -0 in both (exponent None: a zero)
INSIDE = [(0, 0, 1, -14, 0), (0, 0, 2, None, 1), (3, 63, 29, -14, 1), (3, 63, 30, None, 1), (0, 63, 31, -14, 0), (3, 0, 0, None, 1)]


def pos_of(wave, lane, i):
    return wave << 11 | lane << 5 | i


def row_col(wave, lane, i):
    """(row of the pair, column) of value i of a lane: i = 8 k + 4 r + j, float4 column 256 k + 64 wave + lane"""
    return (i >> 2) & 1, 4 * (256 * (i >> 3) + 64 * wave + lane) + (i & 3)


def plant_bits(eb, off, sign):
    if off is None:
        return sign << 31
    return sign << 31 | (eb + off) << 23 | 0x2AAAAA


def plant(pair, eb, n_escapes):
    """pair: (2, 4096) uint32 without escapes -> the first n_escapes of PLANTS and all of INSIDE written into it"""
    for w, lane, i, off, sign in PLANTS[:n_escapes] + INSIDE:
        r, c = row_col(w, lane, i)
        pair[r, c] = plant_bits(eb, off, sign)
    return pair


def lanes_of(pair):
    """(2, 4096) -> (wave, lane, i)"""
    q = pair.reshape(2, 4, 4, 64, 4)             # r, k, wave, lane, j
    return np.ascontiguousarray(q.transpose(2, 3, 1, 0, 4)).reshape(4, 64, 32)


def pair_of(lanes):
    return np.ascontiguousarray(lanes.reshape(4, 64, 4, 2, 4).transpose(3, 2, 0, 1, 4)).reshape(2, 4096)


def escapes(v, eb):
    e = (v >> 23) & 0xFF
    return (e != 0) & (e.astype(np.int64) < eb - 14)


def encode_pair(pair, eb):
    """-> stream (PAIR_DW,), record (REC_DW,), number of escapes"""
    v = lanes_of(pair).astype(np.uint64)
    e = (v >> 23) & 0xFF
    esc = escapes(v, eb)
    c = np.where(e == 0, 0, e.astype(np.int64) - (eb - 15)).astype(np.uint64)
    assert np.all((c[~esc] <= 15))
    t = np.where(esc, 0, (v & 0x807FFFFF) | (c << 23)).astype(np.uint64)
    d = t[..., :LANE_DW].copy()
    for x in range(4):
        p = ((t[..., LANE_DW + x] << 1) | (t[..., LANE_DW + x] >> 31)) & 0x0FFFFFFF
        for q in range(7):
            d[..., 7 * x + q] |= ((p >> (4 * q)) & 0xF) << 27
    stream = d.reshape(4, 64, 7, 4).transpose(0, 2, 1, 3).reshape(-1).astype(np.uint32)   # wave, plane, lane, dword
    at = np.flatnonzero(esc.reshape(-1))          # the flat index IS pos = wave << 11 | lane << 5 | i
    rec = np.zeros(REC_DW, np.uint32)
    rec[0::2] = NO_ESC
    for k, p in enumerate(at[:MAX_ESC]):
        rec[2 * k], rec[2 * k + 1] = p, v.reshape(-1)[p]
    return stream, rec, len(at)


def decode_pair(stream, rec, eb):
    d = stream.reshape(4, 7, 64, 4).transpose(0, 2, 1, 3).reshape(4, 64, LANE_DW).astype(np.uint64)
    t = np.empty((4, 64, 32), np.uint64)
    t[..., :LANE_DW] = d & 0x87FFFFFF
    for x in range(4):
        p = np.zeros((4, 64), np.uint64)
        for q in range(7):
            p |= ((d[..., 7 * x + q] >> 27) & 0xF) << (4 * q)
        t[..., LANE_DW + x] = ((p >> 1) | (p << 31)) & 0xFFFFFFFF
    f = t.astype(np.uint32).view(np.float32)
    v = np.ldexp(f, eb - 15).astype(np.float32).view(np.uint32).reshape(-1)   # exact: every result is normal or +-0
    for k in range(MAX_ESC):
        if rec[2 * k] != NO_ESC:
            v[rec[2 * k]] = rec[2 * k + 1]
    return pair_of(v.reshape(4, 64, 32))


def window_values(rng, n, eb, zeros=0.1):
    """n values (bits) with exponents E - 14 .. E, some +-0: none an escape"""
    e = rng.integers(max(eb - 14, 1), eb + 1, n)
    e[rng.random(n) < zeros] = 0
    m = rng.integers(0, 1 << 23, n)
    m[e == 0] = 0
    return (rng.integers(0, 2, n) << 31 | e << 23 | m).astype(np.uint32)


PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "packed_w.h"
using namespace l2z;
static uint32_t rng = 2024u;
static uint32_t next() { rng = rng * 1664525u + 1013904223u; return rng; }
static int round_trip(int e_base)
{
    uint32_t v[32], d[pk28::kLaneDw], t[32];
    for (int rep = 0; rep < 500; rep++) {
        for (int i = 0; i < 32; i++) {
            const uint32_t r = next(), e = (uint32_t)e_base - next() % 15u;   // exponents E - 14 .. E
            v[i] = (r & 0x807fffffu) | (e << 23);
            if (next() % 16u == 0) v[i] &= 0x80000000u;                        // +-0
        }
        if (pk28::encode_lane(v, e_base, d) != 0u) return 1;                   // no escape inside the window
        pk28::decode_lane_t(d, t);
        for (int i = 0; i < 32; i++)
            if (pk28::value_of_t(t[i], e_base) != v[i]) return 1;
    }
    return 0;
}
int main(int argc, char **argv)
{
    const int es[] = {15, 31, 100, 127, 254};
    for (int e : es)
        if (round_trip(e)) { printf("round trip failed\n"); return 1; }
    // geometry: every dword of a wave's chunk at exactly one (i, lane)
    std::vector<int> hit(pk28::kChunkDw, 0);
    for (int lane = 0; lane < 64; lane++)
        for (int i = 0; i < pk28::kLaneDw; i++) {
            const int o = pk28::plane_off(i, lane);
            if (o < 0 || o >= pk28::kChunkDw) { printf("plane_off out of the chunk\n"); return 1; }
            hit[o]++;
        }
    for (int h : hit)
        if (h != 1) { printf("plane_off not a bijection\n"); return 1; }
    printf("%d %d %d %d %d\n", pk28::kPairDw * 4, pk28::kChunkDw * 4, pk28::kRecDw * 4, (int)pk28::width_ok(4096),
           (int)(pk28::width_ok(8192) || pk28::width_ok(11008) || pk28::width_ok(4352)));
    // record building: pairs from the file
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int32_t hdr[2];
    if (fread(hdr, 4, 2, in) != 2) return 2;
    std::vector<uint32_t> pair(8192), stream(pk28::kPairDw), back(8192);
    uint32_t rec[pk28::kRecDw];
    for (int c = 0; c < hdr[1]; c++) {
        if (fread(pair.data(), 4, 8192, in) != 8192) return 2;
        const int32_t n = pk28::encode_pair(pair.data(), pair.data() + 4096, hdr[0], stream.data(), rec);
        pk28::decode_pair(stream.data(), rec, hdr[0], back.data(), back.data() + 4096);
        fwrite(&n, 4, 1, out);
        fwrite(stream.data(), 4, stream.size(), out);
        fwrite(rec, 4, pk28::kRecDw, out);
        fwrite(back.data(), 4, 8192, out);
    }
    fclose(in);
    fclose(out);
    return 0;
}
"""

CASES = (0, 1, 8, 9)


def test_header_under_sanitizers_against_the_numpy_statement(tmp_path):
    src = tmp_path / "pk28.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "pk28")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", exe], check=True, capture_output=True, text=True)
    rng = np.random.default_rng(28)
    for eb in (31, 127, 254):
        pairs = [plant(window_values(rng, 8192, eb).reshape(2, 4096), eb, n) for n in CASES]
        fin, fout = tmp_path / f"in{eb}.bin", tmp_path / f"out{eb}.bin"
        with open(fin, "wb") as f:
            f.write(np.array([eb, len(pairs)], np.int32).tobytes())
            for p in pairs:
                f.write(p.tobytes())
        run = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        assert run.stdout.split() == ["28672", "7168", "64", "1", "0"]
        got = np.fromfile(fout, np.uint32).reshape(len(pairs), 1 + PAIR_DW + REC_DW + 8192)
        for n, p, g in zip(CASES, pairs, got):
            stream, rec, count = encode_pair(p, eb)
            assert count == n == int(g[0]), (eb, n)                          # 9: overflow, the slot stays at 29 bits
            assert np.array_equal(g[1:1 + PAIR_DW], stream), (eb, n)
            assert np.array_equal(g[1 + PAIR_DW:1 + PAIR_DW + REC_DW], rec), (eb, n)
            want_pos = sorted(pos_of(w, lane, i) for w, lane, i, _, _ in PLANTS[:n])[:MAX_ESC]
            assert [int(x) for x in rec[0:2 * len(want_pos):2]] == want_pos      # sorted by pos, E - 14 and -0 not among them
            assert np.all(rec[2 * len(want_pos)::2] == NO_ESC) and np.all(rec[2 * len(want_pos) + 1::2] == 0)
            for w, lane, i, off, sign in PLANTS[:n]:
                if pos_of(w, lane, i) not in want_pos:   # the ninth in pos order: past the record
                    continue
                k = want_pos.index(pos_of(w, lane, i))
                assert int(rec[2 * k + 1]) == plant_bits(eb, off, sign)
                # an escape's place in the stream holds +0
                if i < LANE_DW:
                    assert int(stream[w * CHUNK_DW + (i // 4) * 256 + lane * 4 + i % 4]) & 0x87FFFFFF == 0
            if n <= MAX_ESC:
                assert np.array_equal(g[1 + PAIR_DW + REC_DW:].reshape(2, 4096), p), (eb, n)
                assert np.array_equal(decode_pair(stream, rec, eb), p), (eb, n)


def test_numpy_round_trip_of_random_lanes():
    rng = np.random.default_rng(7)
    for eb in (15, 31, 100, 127, 200, 254):
        p = window_values(rng, 8192, eb).reshape(2, 4096)
        p[0, 0] = eb << 23   # the matrix maximum sits in this pair
        stream, rec, count = encode_pair(p, eb)
        assert count == 0 and np.all(rec[0::2] == NO_ESC)
        assert stream.size * 4 == 28672
        assert np.array_equal(decode_pair(stream, rec, eb), p), eb


def test_knob_and_hook_are_where_the_abi_says(B):
    tn = open(os.path.join(CSRC, "tunables.cpp")).read()
    assert 'env_int("L2Z_PACKED_BITS", &t.packed_bits)' in tn and '{"L2Z_PACKED_BITS", &t.packed_bits}' in tn
    th = open(os.path.join(CSRC, "tunables.h")).read()
    assert "int packed_bits = 28;" in th and "int packed28_kinds = 40;" in th
    assert 'env_int("L2Z_PACKED28_KINDS", &t.packed28_kinds)' in tn and '{"L2Z_PACKED28_KINDS", &t.packed28_kinds}' in tn
    B.option_set("L2Z_PACKED_BITS", 29)
    B.option_set("L2Z_PACKED_BITS", 28)
    assert "l2z_weights_packed_bits_kind" in B.declared_symbols("test")
    assert "l2z_weights_packed_bits_kind" not in B.declared_symbols("product")
