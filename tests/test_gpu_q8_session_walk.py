"""Seeded random walks over every way the int8 group-quantized family moves a sequence -- l2z_transformer, the greedy and
the sampled loop, l2z_prefill_q8, l2z_transformer_batch_q8, l2z_verify_q8, speculate_q8, forks, rewinds, re-created
runstates and runstates that change to weights of another group size --, each call held to the model of
tests/q8_session_model.py: values against the float64 reference under the family's standing rule, ids, the
bit-for-bit footprint of every call on all 20 runstates, the verify rows, the documented refusals.

The walks are those tests/test_q8_session_walk_cpu.py runs dry (and picks the seeds for); each asserts the coverage on its
own statistics and that its operation counts are the dry walk's.  Measured on an MI355X: profiles/q8_session_walk.md."""
import pytest

import q8_session_model as qm
from test_q8_session_walk_cpu import LIVE_EXCEPTIONS, SEEDS, SPLIT_POS, SPLIT_WALK, WALKS, dry_walk

pytestmark = pytest.mark.gpu

_worlds = {}


@pytest.fixture(scope="module")
def world(gpu, pkg):
    def get(name):
        if name not in _worlds:
            _worlds[name] = qm.World(pkg, name, gpu=gpu)
        return _worlds[name]
    yield get
    for w in _worlds.values():
        w.close()
    _worlds.clear()


def walk(world, pkg, name, seed):
    st = qm.run(world(name), seed, log=print)
    print(f"walk {name} seed {seed}: {st['calls']} operations in {st['wall']:.2f} s, worst deviation {st['worst']:.3e} of the scale "
          f"({st['worst_at']}), {st['exceptions']} exceptions of {st['rows']} rows ({100 * st['exc_share']:.2f} %), "
          f"{st['id_under']} of {st['id_total']} ids under the margin ({st['id_exc']} on exception rows), "
          f"{st['blind_soft']} of {st['blind_total']} mid-loop ids off the reference's under the loose margin, "
          f"{st['end_exceptions']} of {st['end_rows']} end rows over the parity bar, "
          f"operations {dict(st['ops'])}, refusals {dict(st['refusals'])}")
    assert qm.coverage(st) == []   # what the dry walks hold, on what really ran
    assert qm.counts(st) == qm.counts(dry_walk(pkg, name, seed))
    assert st["exc_share"] <= LIVE_EXCEPTIONS, (st["exceptions"], st["rows"])
    assert st["soft_share"] <= LIVE_EXCEPTIONS, (st["blind_soft"], st["blind_total"])   # (tests/test_q8_session_walk_cpu.py)
    return st


@pytest.mark.parametrize("name,seed", WALKS)
def test_q8_session_walk(world, pkg, name, seed):
    walk(world, pkg, name, seed)


def test_q8_session_walk_across_graph_variants(world, pkg, options):
    options(L2Z_ATTN_SPLIT_POS=SPLIT_POS)
    st = walk(world, pkg, *SPLIT_WALK)
    assert qm.split_coverage(st, SPLIT_POS) == []


def test_q8_session_walk_in_several_chunks(world, pkg, options):
    options(L2Z_PF_CHUNK=16)
    walk(world, pkg, "kv24", SEEDS["kv24"][1])
