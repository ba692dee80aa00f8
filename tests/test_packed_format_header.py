"""csrc/packed_w.h itself, compiled for the host: encode_lane / decode_lane_t round-trip bit-exactly for every step count,
and steps / chunk_off / pair_dw agree with each other and with the numpy statement of tests/test_packed_format.py at the
widths the row kernel's paths split on -- n = 4096 (one full batch), 8192 (two), 11008 (a partial last batch), 4352 (a
last batch that gives wave 0 one step and waves 1-3 none)."""
import os
import subprocess

from test_packed_format import lane_dw, pair_dw, steps

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "llama2.zig_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "packed_w.h"
using namespace l2z;
static uint32_t rng = 12345u;
static uint32_t next() { rng = rng * 1664525u + 1013904223u; return rng; }
template <int S> static int round_trip(int e_base)
{
    uint32_t v[8 * S], d[pk::lane_dw(S)], t[8 * S];
    for (int rep = 0; rep < 500; rep++) {
        for (int i = 0; i < 8 * S; i++) {
            const uint32_t r = next(), e = (uint32_t)e_base - next() % 31u;   // exponents E - 30 .. E
            v[i] = (r & 0x807fffffu) | (e << 23);
            if (next() % 16u == 0) v[i] &= 0x80000000u;                        // +-0
        }
        for (int i = 0; i < pk::lane_dw(S); i++) d[i] = 0;
        pk::encode_lane<S>(v, e_base, d);
        pk::decode_lane_t<S>(d, t);
        for (int i = 0; i < 8 * S; i++) {
            // T -> value: the code back to the exponent (what ldexp(T, E - 31) does), 0 stays 0
            const uint32_t c = (t[i] >> 23) & 0xffu;
            const uint32_t back = c == 0 ? (t[i] & 0x80000000u) : ((t[i] & 0x807fffffu) | ((c + (uint32_t)e_base - 31u) << 23));
            if (back != v[i]) return 1;
        }
    }
    return 0;
}
int main()
{
    const int es[] = {31, 100, 127, 254};
    for (int e : es)
        if (round_trip<1>(e) || round_trip<2>(e) || round_trip<3>(e) || round_trip<4>(e)) { printf("round trip failed\n"); return 1; }
    const int ns[] = {4096, 8192, 11008, 4352};
    for (int n : ns) {
        const int n4 = n / 4, nb = (n4 + pk::kBatchF4 - 1) / pk::kBatchF4;
        printf("%d %d %zu", n, (int)pk::width_ok(n), pk::pair_dw(n4));
        for (int b = 0; b < nb; b++)
            for (int w = 0; w < 4; w++) printf(" %d:%zu", pk::steps(n4, b, w), pk::chunk_off(n4, b, w));
        printf("\n");
    }
    return 0;
}
"""


def test_header_round_trips_and_its_geometry_is_consistent(tmp_path):
    src = tmp_path / "pk.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "pk")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I", CSRC, str(src), "-o", exe], check=True,
                   capture_output=True, text=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(out) == 4
    for line, n in zip(out, (4096, 8192, 11008, 4352)):
        f = line.split()
        n4, nb = n // 4, (n // 4 + 1023) // 1024
        assert int(f[0]) == n and int(f[1]) == 1
        assert int(f[2]) == pair_dw(n4)
        chunks = [tuple(int(x) for x in c.split(":")) for c in f[3:]]
        assert len(chunks) == 4 * nb
        off = 0
        for i, (s, o) in enumerate(chunks):   # chunks follow each other in (batch, wave) order, each lane_dw(steps) * 64 dwords
            assert s == steps(n4, i // 4, i % 4)
            assert o == off
            off += 64 * lane_dw(s)
        assert off == pair_dw(n4)
        assert sum(s for s, _ in chunks) * 64 == n4       # every float4 column of a row in exactly one step
    assert [s for s, _ in [tuple(int(x) for x in c.split(":")) for c in out[3].split()[3:]][4:]] == [1, 0, 0, 0]
