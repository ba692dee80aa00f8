"""The session walks of tests/kv8_session_model.py run DRY, without a GPU: ref_q8's "f32" mode stands in the device's place
behind a DryGpu8 that knows kv8 runstates, and is held to the "f64" mode, to its shadows and to the footprint by the same
checks the device gets.  What is tested here is the walk itself -- its schedule is a function of the seed, it reaches every
operation, refusal and edge that kv8_session_model.coverage lists, its exact tier catches a planted error -- and that the
reference alone stays well inside the caps the live walks are held to (tests/test_q8_session_walk_cpu.py's figures): at most
2 % of the compared rows are exceptions (live: 5 %), at most 5 % of the id comparisons fall under the margin.

HOW THE SEEDS WERE PICKED: seeds 1 .. 24 were run dry on each world.  A seed qualified if its walk held and its coverage list
was empty; the two qualifying seeds of a world with the smallest exception share were taken.  The shares of the sweep:
profiles/kv8_session_walk.md."""
import numpy as np
import pytest

import kv8_session_model as km
import ref_q8
from kv8_cases import Kv8Rows
from test_q8_session_walk_cpu import DRY_EXCEPTIONS, LIVE_EXCEPTIONS, UNDER_MARGIN  # noqa: F401

SEEDS = {"kv24": (19, 20), "kv24-v8k": (8, 17), "hs64": (8, 15)}
CHUNK_WALK = ("hs64", SEEDS["hs64"][0], 16)   # under L2Z_PF_CHUNK=16 every chunk takes the row form: the exact tier throughout
WALKS = [(world, seed) for world in km.WORLDS for seed in SEEDS[world]]

_worlds, _stats = {}, {}


def dry_world(pkg, name, pf_chunk=0):
    if (name, pf_chunk) not in _worlds:
        _worlds[name, pf_chunk] = km.World(pkg, name, pf_chunk=pf_chunk)
    return _worlds[name, pf_chunk]


def dry_walk(pkg, name, seed, pf_chunk=0):
    """the statistics of the dry walk, each walked once a process (the GPU file compares its counts with them)"""
    if (name, seed, pf_chunk) not in _stats:
        _stats[name, seed, pf_chunk] = km.run(dry_world(pkg, name, pf_chunk), seed)
    return _stats[name, seed, pf_chunk]


def report(what, st):
    print(f"{what}: {st['calls']} operations in {st['wall']:.2f} s, {st['exceptions']} exceptions of {st['rows']} rows "
          f"({100 * st['exc_share']:.2f} %), worst {st['worst']:.3e} of the scale ({st['worst_at']}), {st['flips']} byte flips, "
          f"{st['moved_rows']} rows moved before they were stored, {st['id_under']} of {st['id_total']} ids under the margin, "
          f"{st['exact_rows']} rows against the shadows ({st['shadow_steps']} shadow steps, {st['exact_skipped']} checks skipped), "
          f"{st['end_exceptions']} of {st['end_rows']} end rows over the parity bar, operations {dict(st['ops'])}, "
          f"refusals {dict(st['refusals'])}")


@pytest.mark.parametrize("world,seed", WALKS)
def test_the_dry_walk_holds_and_covers_everything(pkg, world, seed):
    st = dry_walk(pkg, world, seed)
    report(f"dry walk {world} seed {seed}", st)
    assert len(st["log"]) == km.N_OPS + 1
    assert km.coverage(st, dry_world(pkg, world)) == []
    assert st["exc_share"] <= DRY_EXCEPTIONS, (st["exceptions"], st["rows"])
    assert st["id_total"] >= 20 and st["under_share"] <= UNDER_MARGIN, (st["id_under"], st["id_total"])
    assert st["rows"] >= 1000 and st["end_rows"] >= 2 * km.N_SEQ
    # head size 24 never takes the matrix cores; at head size 64 most histories hold a matrix-core chunk (the chunked walk)
    assert st["exact_rows"] >= 1000 and st["exact_skipped"] == 0 or world == "hs64" and st["exact_rows"] > 0


def test_the_chunked_walk_holds_the_exact_tier_throughout(pkg):
    world, seed, chunk = CHUNK_WALK
    st = dry_walk(pkg, world, seed, chunk)
    report(f"dry walk {world} seed {seed} in chunks of {chunk}", st)
    assert km.coverage(st, dry_world(pkg, world, chunk)) == []
    assert st["exact_skipped"] == 0 and st["flash_chunks"] == 0 and st["chunks_max"] >= 9
    assert st["exc_share"] <= DRY_EXCEPTIONS, (st["exceptions"], st["rows"])


def test_the_schedule_is_a_function_of_the_seed(pkg):
    world, seed = WALKS[0]
    again = km.run(km.World(pkg, world), seed)
    first = dry_walk(pkg, world, seed)
    assert again["log"] == first["log"] and km.counts(again) == km.counts(first)
    assert km.schedule(first) != km.schedule(dry_walk(pkg, world, SEEDS[world][1]))


def test_stop_at_replays_a_prefix(pkg):
    world, seed = WALKS[0]
    whole = dry_walk(pkg, world, seed)["log"]
    part = km.run(km.World(pkg, world), seed, stop_at=20)["log"]
    assert part[-1]["op"] == "end" and 21 <= len(part) - 1 <= 22
    assert part[:-1] == whole[: len(part) - 1]


def test_the_dry_device_is_not_the_reference(pkg):
    """the walk compares two arithmetics: over the committed walks some row left the parity bar and some stored byte landed
    on the other side of a rounding boundary"""
    assert sum(dry_walk(pkg, w, s)["exceptions"] for w, s in WALKS) > 0
    assert sum(dry_walk(pkg, w, s)["flips"] for w, s in WALKS) > 0


def test_the_dry_kv8_runstate_reads_as_kv8_rows_do(pkg):
    """read_kv8 gives the rule's bytes and scales of what was stored, read the values Kv8Rows gives back; a quantizing fork
    the rule's bytes of the source's f32 rows"""
    W = dry_world(pkg, "kv24")
    cfg, w, hs = W.cfg, W.w["a"], W.cfg.head_size
    s8, s32, plain = W.gpu.RunState(cfg, kv8=True), W.gpu.RunState(cfg), Kv8Rows((cfg.n_layers, cfg.seq_len, cfg.kv_dim), hs, np.float32)
    toks = [1, 7, 19, 200, 33]
    s8.prefill_kv8(toks, 0, w)
    s32.prefill_q8(toks, 0, w)
    n = cfg.seq_len * cfg.kv_dim
    for l in range(cfg.n_layers):
        q, s = s8.read_kv8("k", l, 0, len(toks))
        assert q.dtype == np.int8 and q.shape == (len(toks), cfg.kv_dim) and s.shape == (len(toks), cfg.n_kv_heads)
        assert np.abs(q).max(axis=1).min() == 127
        got = s8.read("key_cache", l * n, len(toks) * cfg.kv_dim).reshape(len(toks), -1)
        np.testing.assert_array_equal(got, km.deq(q, s, hs))
    np.testing.assert_array_equal(s8.read("key_cache", 0, cfg.kv_dim), s8.kc[0, 0])
    plain[0, 0] = s32.kc[0, 0]   # (layer 0 does not depend on the attention: the f32 runstate's row through the rule)
    np.testing.assert_array_equal(plain[0, 0], s8.kc[0, 0])
    dst = W.gpu.RunState(cfg, kv8=True)
    W.gpu.runstate_fork(dst, s32, 3)
    for l in range(cfg.n_layers):
        q_want, s_want = ref_q8.quantize_act(s32.vc[l, :3], hs)
        q, s = dst.read_kv8("v", l, 0, 3)
        np.testing.assert_array_equal(q.reshape(-1), q_want)
        np.testing.assert_array_equal(s.reshape(-1), s_want)
    assert not dst.read_kv8("v", 0, 3, 2)[0].any() and np.array_equal(dst.logits(), s32.logits())


# ---- the exact tier catches a planted error (dry only: nothing is planted on the device) ------------------------------
class WrongByte(km.DryState8):
    """a prompt pass that leaves one byte of row 130 in row 2's place"""

    def prefill_kv8(self, tokens, pos0, w):
        super().prefill_kv8(tokens, pos0, w)
        if pos0 <= 2 and pos0 + len(tokens) > 130:
            j = int(np.flatnonzero(self.kc.q[0, 130] != self.kc.q[0, 2])[0])
            row = self.kc.q[0, 2].copy()
            row[j] = self.kc.q[0, 130, j]
            self.kc.take((0, 2), row, self.kc.s[0, 2])


class SecondSliceAtTheFirstOnes(km.DryState8):
    """a prompt pass whose rows from 128 on go to the positions of the first slice of 128"""

    def prefill_kv8(self, tokens, pos0, w):
        for i, t in enumerate(tokens):
            self.transformer(t, pos0 + i % km.WIDE_MAX, w)


@pytest.mark.parametrize("state", [WrongByte, SecondSliceAtTheFirstOnes])
def test_the_shadow_rule_catches_a_planted_error(pkg, state):
    """Both errors stay inside the call's own positions, where the footprint has nothing to say, and the first one moves a
    value by one step of its row: it is the shadow, which steps the same history alone, that tells them"""
    world, seed = WALKS[0]
    log = dry_walk(pkg, world, seed)["log"]
    k = next(e["i"] for e in log if e["op"] == "prefill_kv8" and e["pos"] <= 2 and e["pos"] + e["n"] > 130)

    class Planted(km.DryGpu8):
        State8 = state
    with pytest.raises(km.WalkFailure) as e:
        km.run(km.World(pkg, world, dry_gpu=Planted), seed, stop_at=k)
    assert e.value.index == k, e.value
    assert any("are not its shadow's" in msg for i, msg in e.value.failures if i == k), e.value.failures
    assert not any("changed outside the call's range" in msg for _, msg in e.value.failures)


def test_the_adversarial_fill_keeps_its_dominant_keys_at_the_long_shapes():
    """tests/test_gpu_kv8_prefill.py's "adversarial" fill at the spans added for the two-slice row form and the four-tile
    matrix-core form: for every head the two planted keys stand at least 60 above every other one a query sees, the second
    twice as high as the first"""
    import test_gpu_kv8_prefill as tp
    new = [c for c in tp.KERNEL_CASES if c[4:] not in tp.SPANS]
    assert sorted(set(c[4:] for c in new)) == [(0, 150), (0, 200), (20, 140)] and len(new) == 7
    for form, H, KVH, hs, pos0, P in new:
        q, k8, ks, _, _ = tp.kernel_inputs(H, KVH, hs, pos0, P, "adversarial")
        ks = np.nan_to_num(ks)
        for h in range(H):
            g = h // (H // KVH)
            s = (q[:, h * hs:(h + 1) * hs].astype(np.float64) @ (k8[g].astype(np.float64) * ks[g, :, None]).T) / np.sqrt(hs)
            first, second = 1, pos0 + P // 2
            rest = np.delete(s, [first, second], axis=1)
            assert s[:, first].min() - rest.max() >= 60.0 and np.all(s[:, second] >= 2 * s[:, first] - 1e-9)


def test_the_form_rule_of_the_wide_classifier():
    """csrc/q8_host.cpp q8_gemm_form: more than 16 rows and at least one block of 32 weight rows a CU.  On the 256 CUs of an
    MI355X the vocabulary of kv24-v8k is the smallest that takes the register-blocked form, kv24's takes the tile form"""
    blocks = {name: (km.WORLDS[name][5] + 31) // 32 for name in ("kv24", "kv24-v8k")}
    assert blocks == {"kv24": 9, "kv24-v8k": 256}
