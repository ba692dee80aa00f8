"""Seeded random walks over every way the int8 family moves a sequence ON INT8 KV ROWS -- l2z_prefill_kv8 from one row to
the whole context, l2z_transformer_wide_q8 on up to 128 runstates of either kind, forks of all three kinds onto used
destinations, rewinds, re-created runstates of either kind and a change of weights --, each call held to the model of
tests/kv8_session_model.py: the bit-for-bit footprint on all 150 runstates, every carrier's rows against a
shadow that steps the same history one token at a time, values against the float64 reference with int8 rows, ids, and the
documented refusals.

The walks are those tests/test_kv8_session_walk_cpu.py runs dry (and picks the seeds for); each asserts the coverage on its
own statistics and that its operation counts are the dry walk's.  Measured on an MI355X: profiles/kv8_session_walk.md."""
import pytest

import kv8_session_model as km
from test_kv8_session_walk_cpu import CHUNK_WALK, LIVE_EXCEPTIONS, WALKS, dry_walk, report

pytestmark = pytest.mark.gpu

_worlds = {}


@pytest.fixture(scope="module")
def world(gpu, pkg):
    def get(name, pf_chunk=0):
        if (name, pf_chunk) not in _worlds:
            _worlds[name, pf_chunk] = km.World(pkg, name, gpu=gpu, pf_chunk=pf_chunk)
        return _worlds[name, pf_chunk]
    yield get
    for w in _worlds.values():
        w.close()
    _worlds.clear()


def walk(gpu, world, pkg, name, seed, pf_chunk=0):
    W = world(name, pf_chunk)
    for n in (1, 32, 33, 129, W.cfg.seq_len):   # the model's chunks are the library's own plan
        assert gpu.prefill_plan(n, W.cfg) == W.chunks(n), n
    st = km.run(W, seed, log=print)
    report(f"walk {name} seed {seed}" + (f" in chunks of {pf_chunk}" if pf_chunk else ""), st)
    assert km.coverage(st, W) == []   # what the dry walks hold, on what really ran
    assert km.counts(st) == km.counts(dry_walk(pkg, name, seed, pf_chunk))
    assert st["exc_share"] <= LIVE_EXCEPTIONS, (st["exceptions"], st["rows"])
    return st


@pytest.mark.parametrize("name,seed", WALKS)
def test_kv8_session_walk(gpu, world, pkg, name, seed):
    st = walk(gpu, world, pkg, name, seed)
    assert st["exact_skipped"] == 0 or name == "hs64"


def test_kv8_session_walk_in_several_chunks(gpu, world, pkg, options):
    """l2z_prefill_kv8 cuts its chunks by l2z_prefill_q8's plan: under L2Z_PF_CHUNK=16 every chunk of the head size 64 shape
    takes the row form, so the whole walk is held to the shadows"""
    name, seed, chunk = CHUNK_WALK
    options(L2Z_PF_CHUNK=chunk)
    st = walk(gpu, world, pkg, name, seed, chunk)
    assert st["exact_skipped"] == 0 and st["flash_chunks"] == 0
