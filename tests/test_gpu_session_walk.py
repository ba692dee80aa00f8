"""Seeded random walks over every entry point of the library on a handful of live sequences, each call held to the model of
tests/session_model.py: values against the CPU oracle at the suite's standing bar, ids, the bit-for-bit
footprint of every call on all 24 runstates, the page tables, the documented refusals.

The walks are those tests/test_session_walk_cpu.py runs dry (and picks the seeds for).  L2Z_PF_X3=2 puts every product of the
prompt passes on the bf16 cores, so the planes flags of the runstates are live on these small models; L2Z_PF_CHUNK=32 cuts
the prompt calls into several chunks; L2Z_ATTN_SPLIT_POS=8 puts the switch between the attention graph variants of the
stepped and looped calls where those calls really cross it (asserted on the walk's own statistics).

Measured on an MI355X: profiles/session_walk.md (wall time per walk, err / bar, under-margin shares, the mutation table)."""
import pytest

import session_model as sm
from test_session_walk_cpu import SEEDS, SPLIT_POS, WALKS

pytestmark = pytest.mark.gpu

_worlds = {}


@pytest.fixture(scope="module")
def world(gpu, ck, orc):
    def get(shape):
        if shape not in _worlds:
            _worlds[shape] = sm.World(ck, orc, shape, gpu=gpu)
        return _worlds[shape]
    yield get
    for w in _worlds.values():
        w.close()
    _worlds.clear()


def walk(world, shape, seed):
    st = sm.run(world(shape), seed, log=print)
    print(f"walk {shape} seed {seed}: {st['calls']} operations in {st['wall']:.2f} s, worst err / bar {st['worst']:.3f} "
          f"({st['worst_at']}; logits {st.get('worst_logits', 0):.3f}, KV rows {st.get('worst_kv', 0):.3f}), "
          f"operations {dict(st['ops'])}, {st['id_under']} of {st['id_total']} ids under the margin, refusals {dict(st['refusals'])}")
    assert sm.coverage(st) == []   # what the dry walks hold, on what really ran
    return st


@pytest.mark.parametrize("x3", [1, 2])
@pytest.mark.parametrize("shape,seed", WALKS)
def test_session_walk(world, options, shape, x3, seed):
    options(L2Z_PF_X3=x3)
    walk(world, shape, seed)


def test_session_walk_in_several_chunks(world, options):
    options(L2Z_PF_CHUNK=32)
    walk(world, "hs64", SEEDS["hs64"][1])


def test_session_walk_across_graph_variants(world, options):
    options(L2Z_ATTN_SPLIT_POS=SPLIT_POS)
    st = walk(world, "hs64", SEEDS["hs64"][0])
    assert sm.split_coverage(st, SPLIT_POS) == []
