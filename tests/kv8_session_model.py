"""The third session walk: the int8 family ON INT8 KV ROWS -- l2z_transformer_wide_q8 up to 128 rows,
l2z_prefill_kv8, the kv8 runstates and the quantizing l2z_runstate_fork --, in the shape of tests/q8_session_model.py and on
its plumbing (Walk8 is a q8_session_model.Walk; the f32 walk's rules come through it).  No GPU in this module:
tests/test_kv8_session_walk_cpu.py runs the walks dry (ref_q8's "f32" mode behind a DryGpu8 that knows kv8 runstates),
tests/test_gpu_kv8_session_walk.py on the device.

World: the shapes of WORLDS, two weights objects "a" and "b" each (another one restarts a sequence at position 0);
N_SEQ runstates that carry the sequences (CARRIERS: of either kind, a re-creation may change it), N_FILL8 kv8 and N_FILL32 f32
runstates that only serve as rows of a wide step (no history, no reference: footprint and ids alone); live, f32 weights and
a paged runstate for the refusals.

Per carrier, beside what the q8 walk holds:
    kind    "kv8" or "f32"
    tags    one tag per consumed token, the PROVENANCE of its KV rows: 0 a row the kv8 arithmetic computed (a wide step, the
            prompt pass's row form: the same bits), F > 0 a row of the quantizing fork number F, F < 0 a row
            of the matrix-core chunk number -F (head size 64: chunks of more than 32 rows), which stepping does not reproduce
    ref     the float64 model; on a kv8 carrier its caches are Rows (kv8_cases.Kv8Rows that keep bytes and scales)
    shadow  a kv8 runstate of its own, moved ONLY by transformer_wide_q8 with n = 1, by the quantizing fork from the same
            source the carrier was forked from, and -- where a kv8-from-kv8 fork hands on rows of a quantizing fork, which no
            stepping reproduces -- by the same fork between the two shadows

The checks after every call:
    footprint  every byte and scale (kv8) or f32 row of every layer of every runstate outside the call's positions, and the
               logits of every absent runstate, bit for bit; the spare and the paged runstate included
    exact      the documented invariances make a kv8 carrier's rows a function of (token, tag) history alone, so after a
               call that moved it the shadow is brought to that history and every byte and scale below the depth is the
               shadow's, in every layer; after a wide step the logits are the shadow's bits, after prefill_kv8 they meet the
               parity bar (another classifier launch).  A fork's rows are the source's (kv8 from kv8, f32 from f32) or
               ref_q8.quantize_act of the source's f32 rows as read before the call.  Held while no tag of the history is
               negative (Seq.exact)
    float64    q8_session_model's value rule, with healing the rule in force: a stored byte on the other side of a rounding
               boundary stays in the cache, so after a call with an exception among its K / V rows the reference takes the
               device's rows of the call (bytes and scales).  Where device and reference bytes differ, the position's FIRST
               such layer is classed (Walk8.byte_rule): a flip of the stored row's own rounding -- by exactly 1, the scales
               at the parity bar -- or a row moved before it was stored; the walk counts and logs both
    ids        every want_next id is first_max of the row the device left, the reference's argmax above the margin; every
               sample_batch id the host sampler's
At the end: every row below every carrier's depth once more against shadow and reference; everything closes.
"""
from collections import Counter

import numpy as np

import kv8_prefill_cases
import q8_batch_cases as bc
import q8_cases
import q8_session_model as qm
import ref_q8
from kv8_cases import Kv8Rows
from q8_session_model import ERR_INVALID, ERR_STATE, DryError  # noqa: F401
from session_model import WalkFailure, bits, first_max  # noqa: F401

f32 = np.float32
N_SEQ, N_KV8_FIRST, N_FILL8, N_FILL32 = 8, 6, 128, 12
WIDE_MAX = 128
WORLDS = {"kv24": bc.KV24, "kv24-v8k": bc.KV24[:5] + (8192,) + bc.KV24[6:], "hs64": kv8_prefill_cases.SHAPE}
HS64_SEED = 1   # (the walks heal: they need no checkpoint on which the reference's two modes agree everywhere)
N_OPS = 84   # (the q8 walks' 120 with a shadow step per moved position took three times their time)
N_CLASSES = ((1, 1), (2, 16), (17, 64), (65, 128))
ROW_CLASSES = ((1, 1), (2, 32), (33, 64), (65, 128), (129, None))
EDGES = (64, 128)
FLASH_ROWS = 32   # kv8.h kv8_prefill_flash_shape: head size 64 or 128 and MORE rows than this take the matrix cores
KV8_ENTRIES = ("l2z_transformer", "l2z_prefill", "l2z_prefill_q8", "l2z_transformer_batch_q8", "l2z_verify_q8",
               "l2z_transformer_wide", "l2z_step_mixed", "l2z_score")   # tests/test_kv8_abi.py REFUSED, the entry points
REFUSED_CALLS = {
    "kv8_entry": KV8_ENTRIES, "mixed_kind": ("a mixed-kind call",),
    "fork_kinds": ("fork into an f32 runstate", "fork into a paged runstate", "fork from a paged runstate"),
    "prefill_kv8_wrong": ("an f32 runstate", "a paged runstate", "f32 weights"),
    "past_end": ("prefill_kv8", "transformer_wide_q8"), "bad_token": ("prefill_kv8", "transformer_wide_q8"),
    "duplicate": ("transformer_wide_q8",), "rows129": ("transformer_wide_q8",)}
REFUSALS = tuple(REFUSED_CALLS)
OP_KINDS = ("prefill_kv8", "prefill_q8", "wide_kv8", "wide_f32", "fork_88", "fork_832", "fork_3232", "trim", "rewind", "recreate",
            "reweight", "argmax", "argmax_batch", "sample_batch", "probs", "logits", "write_logits")


class Rows(Kv8Rows):
    """Kv8Rows that keep what they store: q int8 like the rows, s f32 [..., kv heads]"""

    def __init__(self, shape, head_size, ft):
        super().__init__(shape, head_size, ft)
        self.q, self.s = np.zeros(shape, np.int8), np.zeros(shape[:-1] + (shape[-1] // head_size,), f32)

    def __setitem__(self, at, row):
        q, s = ref_q8.quantize_act(np.asarray(row).astype(f32), self.hs)
        self.q[at], self.s[at] = q.reshape(self.q[at].shape), s.reshape(self.s[at].shape)
        self.a[at] = self.q[at].astype(f32) * np.repeat(self.s[at], self.hs, axis=-1)

    def take(self, at, q, s):
        """the rows `at` become the stored bytes q and scales s"""
        self.q[at], self.s[at] = q, s
        self.a[at] = np.asarray(q).astype(f32) * np.repeat(np.asarray(s, f32), self.hs, axis=-1)


def deq(q, s, hs):
    return q.astype(f32) * np.repeat(s, hs, axis=-1)


# ---- the dry device -------------------------------------------------------------------------------------------------------
class DryState8(qm.DryState):
    """a kv8 runstate of the dry device: the f32 pass over Rows"""
    kv8 = True

    def __init__(self, gpu, cfg):
        super().__init__(gpu, cfg)
        self.kc, self.vc = (Rows(self.kc.shape, cfg.head_size, f32) for _ in range(2))

    def prefill_kv8(self, tokens, pos0, w):
        for i, t in enumerate(tokens):
            self.transformer(t, pos0 + i, w)

    def read_kv8(self, which, layer, pos0, n_pos):
        r = self.kc if which == "k" else self.vc
        return r.q[layer, pos0:pos0 + n_pos].copy(), r.s[layer, pos0:pos0 + n_pos].copy()

    def read(self, name, offset, count):
        return (self.kc if name == "key_cache" else self.vc).a.reshape(-1)[offset:offset + count].copy()


class DryGpu8(qm.DryGpu):
    State8 = DryState8

    def RunState(self, cfg, kv8=False):
        return self.State8(self, cfg) if kv8 else qm.DryState(self, cfg)

    def transformer_wide_q8(self, states, tokens, pos, w, want_next=True):
        for s, t, p in zip(states, tokens, pos):
            s.transformer(t, p, w)
        return np.array([s.argmax() for s in states], np.int32) if want_next else None

    def runstate_fork(self, dst, src, n_pos):
        d8, s8 = getattr(dst, "kv8", False), getattr(src, "kv8", False)
        if not d8:
            return super().runstate_fork(dst, src, n_pos)
        for d, s in ((dst.kc, src.kc), (dst.vc, src.vc)):
            if s8:
                d.take(np.s_[:, :n_pos], s.q[:, :n_pos], s.s[:, :n_pos])
            else:
                d[:, :n_pos] = s[:, :n_pos]
        dst.z = src.z.copy()


# ---- the world ------------------------------------------------------------------------------------------------------------
class World:
    """what the walks of one shape share; gpu=None: a dry world.  pf_chunk: the L2Z_PF_CHUNK the live walk runs under (0: a
    prompt of these lengths is ONE chunk, which the live test asserts on the library's own plan)"""

    def __init__(self, pkg, name, gpu=None, dry_gpu=None, pf_chunk=0):
        ck = pkg.checkpoint
        self.name, self.live, self.B, self.pf_chunk = name, gpu is not None, pkg.binding, pf_chunk
        shp = WORLDS[name]
        self.cfg = ck.Config(*shp[:7])
        self.H = qm.host_sampler()
        self.gpu = gpu if gpu is not None else (dry_gpu or DryGpu8)(self.H)
        seed = HS64_SEED if name == "hs64" else bc.KV24_SEED
        blobs = {k: ck.synth_blob(self.cfg, True, seed + i) for i, k in enumerate("ab")}
        self.gs = {"a": shp[7], "b": shp[7]}
        self.blob = blobs["a"]
        self.body = {k: ck.v2_body_from_f32(self.cfg, blobs[k], True, self.gs[k]) for k in "ab"}
        self.t = {k: ck.v2_carve(self.cfg, self.body[k], True, self.gs[k]) for k in "ab"}
        if self.live:
            self.w = {k: gpu.Weights.from_q8(self.cfg, self.body[k], True, self.gs[k]) for k in "ab"}
            self.w32 = gpu.Weights(self.cfg, self.blob, True)
        else:
            self.w = {k: qm.DryWeights(self.cfg, self.t[k], self.gs[k]) for k in "ab"}
            self.w32 = None

    def chunks(self, n):
        """the lengths of the chunks a prompt pass of n rows runs in"""
        c = self.pf_chunk
        return [n] if c <= 0 else [c] * (n // c) + ([n % c] if n % c else [])

    close = qm.World.close


class Seq(qm.Seq):
    def __init__(self, idx):
        super().__init__(idx)
        self.name = ("s" if idx < N_SEQ else "x" if idx < N_SEQ + N_FILL8 else "y") + str(idx)
        self.kind = self.shadow = self.shadow_seq = self.swk = None
        self.spairs = []

    def reset(self):
        self.hist, self.tags, self.zref, self.next_tok, self.snap, self.flash_end = [], [], None, None, None, None

    @property
    def exact(self):
        return self.kind == "kv8" and not any(t < 0 for t in self.tags)

    def pairs(self):
        return list(zip(self.hist, self.tags))


def caches(snap):
    return [k for k in snap if k not in ("z", 0)]


def klass(n, classes):
    return next(i for i, (lo, hi) in enumerate(classes) if n >= lo and (hi is None or n <= hi))


class Walk8(qm.Walk):
    AFTER = qm.Walk.AFTER + ("write_logits",)
    MAIN = (("prefill_kv8", 12), ("prefill_q8", 4), ("wide_kv8", 12), ("wide_f32", 4), ("fork_88", 4), ("fork_832", 4),
            ("fork_3232", 2), ("trim", 1), ("recreate", 3), ("reweight", 3))

    def __init__(self, world, seed, n_ops=N_OPS, log=None, stop_at=None):
        super().__init__(world, seed, n_ops=n_ops, log=log, stop_at=stop_at, heal=True)
        self.rng = np.random.default_rng([int(seed), 0x4B38])
        self.seqs = [Seq(i) for i in range(N_SEQ + N_FILL8 + N_FILL32)]
        self.hs, self.kvh = self.cfg.head_size, self.cfg.n_kv_heads
        self.flash = self.hs in (64, 128)
        self.n_tag = self.n_drawn = 0
        self.st.update(n_classes=Counter(), row_classes=Counter(), cont_off64=0, end_at_len=0, wide_last_row=0, zero_beside_deep=0,
                       tail_after_flash=0, flash_high=0, flash_chunks=0, wide17=0, want_next=set(), fork_stale=set(), flips=0, moved_rows=0,
                       exact_rows=0, exact_skipped=0, shadow_steps=0, chunks_max=0)

    # ---- runstates -------------------------------------------------------------------------------------------------------
    def main(self):
        return self.seqs[:N_SEQ]

    def make(self, q, wk, kind=None):
        if kind is None:
            kind = "kv8" if q.idx < N_KV8_FIRST or N_SEQ <= q.idx < N_SEQ + N_FILL8 else "f32"
        q.rs, q.kind = self.gpu.RunState(self.cfg, kv8=kind == "kv8"), kind
        if not q.fill and q.shadow is None:   # (read through a Seq of its own, by the carriers' reader)
            q.shadow, q.shadow_seq = self.gpu.RunState(self.cfg, kv8=True), Seq(-1)
            q.shadow_seq.rs, q.shadow_seq.kind = q.shadow, "kv8"
        q.reset()
        self.bind(q, wk)

    def bind(self, q, wk):
        q.wk, q.hist, q.tags, q.flash_end = wk, [], [], None
        if not q.fill:
            q.ref = ref_q8.Q8Model(self.cfg, self.W.t[wk], self.W.gs[wk], "f64")
            if q.kind == "kv8":
                q.ref.kc, q.ref.vc = (Rows(q.ref.kc.shape, self.hs, q.ref.ft) for _ in range(2))

    def tag(self, sign):
        self.n_tag += 1
        return sign * self.n_tag

    def read(self, q):
        """the bits of a runstate: logits, and per cache the bytes and scales (kv8) or the f32 rows, [layers, seq_len, ...]"""
        c = self.cfg
        snap = dict(z=bits(q.rs.logits()))
        snap[0] = snap["z"]   # (where q8_session_model's logits-only calls look for them)
        if getattr(q, "kind", None) == "kv8":
            for which in "kv":
                rows = [q.rs.read_kv8(which, l, 0, self.L) for l in range(c.n_layers)]
                snap[which + "q"] = np.stack([r[0] for r in rows])
                snap[which + "s"] = bits(np.stack([r[1] for r in rows]))
        else:
            n, shape = c.n_layers * self.L * self.kvd, (c.n_layers, self.L, self.kvd)
            snap["k"] = bits(q.rs.read("key_cache", 0, n)).reshape(shape).copy()
            snap["v"] = bits(q.rs.read("value_cache", 0, n)).reshape(shape).copy()
        return snap

    def rows32(self, snap, which):
        """a snapshot's K or V rows as f32 values (a kv8 one's dequantized)"""
        if which in snap:
            return snap[which].view(f32)
        return deq(snap[which + "q"], snap[which + "s"].view(f32), self.hs)

    def settle(self, touched):
        """after a call: touched = {seq: (lo, hi) rows the call may write, or None: any row}: the footprint"""
        for q in self.seqs + self.others:
            new, old = self.read(q), q.snap
            if old is not None and not (q in touched and touched[q] is None):
                keep = np.ones(self.L, bool)
                if q in touched:
                    keep[touched[q][0]: touched[q][1]] = False
                for name in caches(new):
                    if not np.array_equal(old[name][:, keep], new[name][:, keep]):
                        axes = tuple(i for i in range(old[name].ndim) if i != 1)
                        rows = np.flatnonzero(keep)[np.any(old[name][:, keep] != new[name][:, keep], axis=axes)]
                        self.fail(f"{q.name}: cache rows {rows[:8].tolist()} ({name}) changed outside the call's range "
                                  f"{touched.get(q, 'absent')}")
                if q not in touched and not np.array_equal(old["z"], new["z"]):
                    self.fail(f"{q.name}: logits changed by a call it took no part in")
            q.snap = new

    # ---- the exact tier ------------------------------------------------------------------------------------------------
    def step_shadow(self, q, tok, pos):
        self.gpu.transformer_wide_q8([q.shadow], [int(tok)], [int(pos)], self.W.w[q.wk], want_next=False)
        self.st["shadow_steps"] += 1

    def exact_tier(self, q, logits=None, end=False):
        """bring q's shadow to q's history and hold q's rows below its depth (and its logits: "same" bits, "parity") to it"""
        if not q.exact:
            self.st["exact_skipped"] += 1
            return
        want, d = q.pairs(), len(q.hist)
        if q.swk != q.wk:
            q.spairs, q.swk = [], q.wk
        c = 0
        while c < min(len(want), len(q.spairs)) and want[c] == q.spairs[c]:
            c += 1
        if logits is not None:   # the shadow's logits are to be the last position's: it is stepped again (the same bytes)
            c = min(c, d - 1)
        if any(t != 0 for _, t in want[c:]):
            self.fail(f"{q.name}: rows {c} .. of its history are a fork's and its shadow does not hold them (the model's error)")
            return
        for p in range(c, d):
            self.step_shadow(q, want[p][0], p)
        q.spairs = want
        mine, its = q.snap, self.read(q.shadow_seq)
        for name in ("kq", "ks", "vq", "vs"):
            if not np.array_equal(mine[name][:, :d], its[name][:, :d]):
                rows = np.flatnonzero(np.any(mine[name][:, :d] != its[name][:, :d], axis=(0, 2)))
                self.fail(f"{q.name}: rows {rows[:8].tolist()} ({name}) are not its shadow's, which stepped the same history")
        self.st["exact_rows"] += d
        if logits == "same" and not np.array_equal(mine["z"], its["z"]):
            self.fail(f"{q.name}: its logits are not the bits of its shadow's, which stepped the same token alone")
        if logits == "parity" and not q8_cases.parity_ok(mine["z"].view(f32), its["z"].view(f32)):
            self.fail(f"{q.name}: its logits are {q8_cases.scaled_dev(mine['z'].view(f32), its['z'].view(f32)):.3e} of the scale off "
                      f"its shadow's, over the parity bar")

    # ---- the float64 tier ----------------------------------------------------------------------------------------------
    def byte_rule(self, q, p):
        """position p of a kv8 carrier: the first (layer, K before V) whose bytes differ from the reference's is either a
        FLIP -- every difference is exactly 1 and the row's largest elements (127 s) meet the parity bar: the stored row's own
        rounding -- or a row that was MOVED before it was stored (a quantized activation of an earlier product on the other
        side of a boundary, the family's standing exception).  Both are counted and logged; what holds either is the value
        rule (under LOOSE, and an exception of the capped share): ref_q8's own two modes differ by 2 in a byte at scales that
        meet the bar (hs64, seed 15 of the sweep), so nothing stricter can be asked of the bytes"""
        for l in range(self.cfg.n_layers):
            for which, r in (("k", q.ref.kc), ("v", q.ref.vc)):
                dq, ds = q.snap[which + "q"][l, p], q.snap[which + "s"].view(f32)[l, p]
                diff = np.abs(dq.astype(np.int32) - r.q[l, p].astype(np.int32))
                if diff.any():
                    at = (q.name, p, l, which, int(np.count_nonzero(diff)))
                    if diff.max() == 1 and q8_cases.parity_ok(127.0 * ds, 127.0 * r.s[l, p]):
                        self.st["flips"] += int(np.count_nonzero(diff))
                        self.cur["flips"] = self.cur.get("flips", []) + [at]
                    else:
                        self.st["moved_rows"] += 1
                        self.cur["moved"] = self.cur.get("moved", []) + [at]
                    return

    def feed(self, q, pos0, toks, zrows):
        """q8_session_model.Walk.feed on either kind of carrier; on a kv8 one with the byte rule, and healing takes the
        device's bytes and scales of ALL the call's rows once one of them was an exception"""
        K, V = self.rows32(q.snap, "k"), self.rows32(q.snap, "v")
        kc = q.ref.kc.a if q.kind == "kv8" else q.ref.kc
        vc = q.ref.vc.a if q.kind == "kv8" else q.ref.vc
        zs, oks, hurt = [], {}, False
        for i, t in enumerate(toks):
            p = pos0 + i
            z = q.ref.transformer(int(t), p)
            ok_k = self.compare(f"{q.name} K rows of position {p}", K[:, p], kc[:, p])
            ok_v = self.compare(f"{q.name} V rows of position {p}", V[:, p], vc[:, p])
            if q.kind == "kv8":
                self.byte_rule(q, p)
            if not (ok_k and ok_v):
                hurt = True
                self.heal_rows(q, p, p + 1)
            if i in zrows:
                oks[i] = self.compare(f"{q.name} logits of position {p}", zrows[i], z)
            zs.append(z)
        if hurt:
            self.heal_rows(q, pos0, pos0 + len(toks))
        return zs, oks

    def heal_rows(self, q, lo, hi):
        if q.kind == "kv8":
            for which, r in (("k", q.ref.kc), ("v", q.ref.vc)):
                r.take(np.s_[:, lo:hi], q.snap[which + "q"][:, lo:hi], q.snap[which + "s"].view(f32)[:, lo:hi])
        else:
            q.ref.kc[:, lo:hi], q.ref.vc[:, lo:hi] = q.snap["k"].view(f32)[:, lo:hi], q.snap["v"].view(f32)[:, lo:hi]

    def moved(self, q, pos0, toks, tags, zs):
        q.hist = q.hist[:pos0] + [int(t) for t in toks]
        q.tags = q.tags[:pos0] + list(tags)
        q.zref = zs[-1]

    def place(self, q, n, aim=None):
        """where q's next n rows go -- on from its depth where they fit, now and then a rewind that rewrites rows -- and the
        tokens it is fed there"""
        d = len(q.hist)
        pos0 = d if aim is None else aim
        if aim is None and (d + n > self.L or self.rng.random() < 0.12):
            pos0 = int(self.rng.integers(0, max(min(d, self.L - n), 0) + 1))
            if n == 1 and d == self.L and self.rng.random() < 0.5:   # (a full sequence's step: the last row again)
                pos0 = self.L - 1
        toks = self.rng.integers(2, self.V, n).astype(np.int32)
        if pos0 == 0:
            toks[0] = 1
        elif pos0 == d and q.next_tok is not None and self.rng.random() < 0.7:
            toks[0] = q.next_tok
        if pos0 < d:
            self.cur["rewind"] = self.cur.get("rewind", 0) + 1
        return pos0, toks

    # ---- the prompt passes ---------------------------------------------------------------------------------------------
    def op_prefill_kv8(self, q=None, n=None, pos0=None):
        L = self.L
        if q is None:
            have = [x for x in self.main() if x.kind == "kv8"]
            if not have:
                return False
            q, u = have[int(self.rng.integers(0, len(have)))], self.rng.random()
            tails = [x for x in have if x.flash_end is not None and x.flash_end == len(x.hist) < L]
            room = [x for x in have if len(x.hist) < L - 1]
            mids = [x for x in have if 64 < len(x.hist) <= L - FLASH_ROWS - 1]
            if u < 0.3 and tails:   # a short row-form chunk right behind a matrix-core one
                q = tails[0]
                n, aim = int(self.rng.integers(1, min(FLASH_ROWS, L - len(q.hist)) + 1)), len(q.hist)
            elif u < 0.42 and room:   # ... to the very end of the context
                q = room[int(self.rng.integers(0, len(room)))]
                n, aim = L - len(q.hist), len(q.hist)
            elif u < 0.52 and room:   # ... and one short of it: the next wide step writes the last row
                q = room[int(self.rng.integers(0, len(room)))]
                n, aim = L - 1 - len(q.hist), len(q.hist)
            elif u < 0.62 and mids:   # a chunk of more than 32 rows from above position 64
                q = mids[int(self.rng.integers(0, len(mids)))]
                n, aim = int(self.rng.integers(FLASH_ROWS + 1, L - len(q.hist) + 1)), len(q.hist)
            else:   # every class of row counts in turn
                lo, hi = ROW_CLASSES[(2, 0, 4, 1, 3)[self.n_drawn % len(ROW_CLASSES)]]
                self.n_drawn += 1
                n, aim = int(self.rng.integers(lo, (hi or L) + 1)), None
            pos0, t = self.place(q, n, aim)
        else:
            t = np.append(1, self.rng.integers(2, self.V, n - 1)).astype(np.int32)
        d = len(q.hist)
        self.cur.update(seq=q.name, pos=pos0, n=n)
        q.rs.prefill_kv8(t, pos0, self.w(q))
        st, tags, at, tail = self.st, [], pos0, q.flash_end is not None and q.flash_end == d == pos0
        chunks = self.W.chunks(n)
        for k, c in enumerate(chunks):
            core = self.flash and c > FLASH_ROWS
            tags += [self.tag(-1) if core else 0] * c
            if core:
                st["flash_chunks"] += 1
                st["flash_high"] += at > 64
            elif k == 0 and tail and c <= FLASH_ROWS:
                st["tail_after_flash"] += 1
            tail = core
            at += c
        st["chunks_max"] = max(st["chunks_max"], len(chunks))
        st["row_classes"][klass(n, ROW_CLASSES)] += 1
        st["cont_off64"] += pos0 == d and pos0 % 64 != 0
        st["end_at_len"] += pos0 + n == L
        self.crossed("prefill_kv8", pos0, n)
        self.settle({q: (pos0, pos0 + n)})
        zs, _ = self.feed(q, pos0, t, {n - 1: q.snap["z"].view(f32)})
        self.moved(q, pos0, t, tags, zs)
        q.next_tok, q.flash_end = None, pos0 + n if tail else None
        self.exact_tier(q, "parity")

    def op_prefill_q8(self, q=None, n=None, pos0=None):
        if q is None:
            have = [x for x in self.main() if x.kind == "f32"]
            if not have:
                return False
            q = have[int(self.rng.integers(0, len(have)))]
            n = int(self.rng.integers(1, self.L // 3 + 1))
            pos0, t = self.place(q, n)
        else:
            t = np.append(1, self.rng.integers(2, self.V, n - 1)).astype(np.int32)
        self.cur.update(seq=q.name, pos=pos0, n=n)
        q.rs.prefill_q8(t, pos0, self.w(q))
        self.crossed("prefill_q8", pos0, n)
        self.settle({q: (pos0, pos0 + n)})
        zs, _ = self.feed(q, pos0, t, {n - 1: q.snap["z"].view(f32)})
        self.moved(q, pos0, t, [0] * n, zs)
        q.next_tok = None

    # ---- the wide step -------------------------------------------------------------------------------------------------
    def op_wide(self, kind):
        L = self.L
        fills = self.seqs[N_SEQ: N_SEQ + N_FILL8] if kind == "kv8" else self.seqs[N_SEQ + N_FILL8:]
        k = self.st["ops"]["wide_" + kind]
        lo, hi = N_CLASSES[(3, 0, 2, 1)[k] if k < 4 else int(self.rng.integers(0, len(N_CLASSES)))]
        n = int(self.rng.integers(lo, hi + 1))
        wk = "ab"[int(self.rng.integers(0, 2))]
        mains = [q for q in self.main() if q.kind == kind and q.wk == wk]
        if not mains:
            wk = "ab"[wk == "a"]
            mains = [q for q in self.main() if q.kind == kind and q.wk == wk]
        mains = [mains[i] for i in self.rng.permutation(len(mains))]
        # the carrier that stands one short of the end first, then the deepest, then the shallowest
        mains.sort(key=lambda x: (len(x.hist) != L - 1, -len(x.hist)))
        if len(mains) > 2:
            mains = mains[:1] + mains[-1:] + mains[1:-1]
        m = int(self.rng.integers(min(1, len(mains)), len(mains) + 1))
        n = min(n, m + len(fills))
        qs = mains[: min(max(m, n - len(fills)), n)]
        if not qs and kind == "f32":
            return False
        zero = qs[min(1, len(qs) - 1)] if len(qs) > 1 and self.rng.random() < 0.5 else None   # (the shallowest of them)
        rows = []
        for q in qs:
            p, t = self.place(q, 1, 0 if q is zero else None)
            rows.append((q, p, int(t[0])))
        for f in self.pick(n - len(qs), fills):
            p = int(self.rng.integers(0, 8)) if self.rng.random() < 0.7 else int(self.rng.integers(0, L))
            rows.append((f, p, 1 if p == 0 else int(self.rng.integers(2, self.V))))
        rows = [rows[i] for i in self.rng.permutation(len(rows))]
        want_next = bool(self.rng.random() < 0.5)
        self.cur.update(seqs=[q.name for q, _, _ in rows if not q.fill], n=len(rows), pos=[p for q, p, _ in rows if not q.fill], wk=wk,
                        want_next=want_next)
        nxt = self.gpu.transformer_wide_q8([q.rs for q, _, _ in rows], [t for _, _, t in rows], [p for _, p, _ in rows], self.W.w[wk],
                                           want_next=want_next)
        st, at = self.st, [p for q, p, _ in rows if not q.fill]
        st["n_classes"][klass(len(rows), N_CLASSES)] += 1
        st["want_next"].add(want_next)
        st["wide17"] += len(rows) > 16
        st["wide_last_row"] += any(p == L - 1 for p in at)
        st["zero_beside_deep"] += any(p == 0 for p in at) and any(p >= 128 for p in at)
        self.settle({q: (p, p + 1) for q, p, _ in rows})
        for i, (q, p, t) in enumerate(rows):
            z_dev = q.snap["z"].view(f32)
            if q.fill:
                if want_next and int(nxt[i]) != first_max(z_dev):
                    self.fail(f"{q.name}: id {int(nxt[i])} is not the first maximum {first_max(z_dev)} of the row the device left")
                continue
            zs, oks = self.feed(q, p, [t], {0: z_dev})
            self.moved(q, p, [t], [0], zs)
            q.next_tok, q.flash_end = None, None
            if want_next:
                self.ident(f"{q.name} wide step", nxt[i], z_dev, zs[0], oks[0])
                q.next_tok = int(nxt[i])
            if kind == "kv8":
                self.exact_tier(q, "same")

    def op_wide_kv8(self):
        return self.op_wide("kv8")

    def op_wide_f32(self):
        return self.op_wide("f32")

    # ---- forks ---------------------------------------------------------------------------------------------------------
    def op_fork(self, dkind, skind):
        src = [q for q in self.main() if q.kind == skind and q.zref is not None]
        if not src:
            return False
        s = src[int(self.rng.integers(0, len(src)))]
        dsts = [q for q in self.main() if q is not s and q.kind == dkind]
        if not dsts:
            return False
        depth = len(s.hist)
        name = "fork_" + {"kv8": "8", "f32": "32"}[dkind] + {"kv8": "8", "f32": "32"}[skind]
        rel = ("below", "at", "above")[self.st["ops"][name] % 3]
        if rel == "below" and depth == 0 or rel == "above" and depth == self.L:
            rel = "at"
        n_pos = {"below": int(self.rng.integers(0, max(depth, 1))), "at": depth,
                 "above": int(self.rng.integers(depth + 1, self.L + 1)) if depth < self.L else depth}[rel]
        used = [q for q in dsts if len(q.hist) > n_pos] or [q for q in dsts if q.hist]
        d = (used or dsts)[int(self.rng.integers(0, len(used or dsts)))]
        if 0 < len(d.hist) <= n_pos and self.rng.random() < 0.7:   # a destination with rows of its own beyond the fork's
            n_pos = int(self.rng.integers(0, len(d.hist)))
            rel = "below" if n_pos < depth else "at" if n_pos == depth else "above"
        self.cur.update(dst=d.name, src=s.name, n_pos=n_pos, rel=rel)
        before = s.snap
        self.gpu.runstate_fork(d.rs, s.rs, n_pos)
        self.st["fork_rel"].add(rel)
        if len(d.hist) > n_pos:
            self.st["fork_stale"].add(name)
        keep = min(n_pos, depth)
        if d.wk != s.wk:
            self.bind(d, s.wk)
        d.hist, d.zref, d.next_tok, d.flash_end = s.hist[:keep], s.zref, None, None
        self.settle({d: (0, n_pos)})
        if not np.array_equal(d.snap["z"], s.snap["z"]):
            self.fail(f"{d.name}: its logits are not {s.name}'s after the fork")
        at = np.s_[:, :keep]
        if dkind == skind:   # a copy
            d.tags = s.tags[:keep] if s.exact or dkind == "f32" else [-abs(t) for t in s.tags[:keep]]   # (no shadow holds them)
            for nm in caches(d.snap):
                if not np.array_equal(d.snap[nm][:, :n_pos], before[nm][:, :n_pos]):
                    self.fail(f"{d.name}: cache rows below {n_pos} ({nm}) are not {s.name}'s after the fork")
            if dkind == "kv8":
                for a, b in ((d.ref.kc, s.ref.kc), (d.ref.vc, s.ref.vc)):
                    a.take(at, b.q[at], b.s[at])
            else:
                d.ref.kc[at], d.ref.vc[at] = s.ref.kc[at], s.ref.vc[at]
        else:   # the rule's bytes of the f32 rows as they were read before the call, every layer, all n_pos rows
            d.tags = [self.tag(1)] * keep
            for which, r, rs in (("k", d.ref.kc, s.ref.kc), ("v", d.ref.vc, s.ref.vc)):
                rows = before[which].view(f32)[:, :n_pos]
                q_want, s_want = ref_q8.quantize_act(rows, self.hs)
                if not np.array_equal(d.snap[which + "q"][:, :n_pos].reshape(-1), q_want) or \
                        not np.array_equal(d.snap[which + "s"][:, :n_pos].reshape(-1), bits(s_want)):
                    self.fail(f"{d.name}: {which} rows below {n_pos} are not the rule's bytes and scales of {s.name}'s f32 rows")
                r[at] = rs[at]
            hurt = False
            for p in range(keep):   # ... and against float64: the reference's rows through the rule
                ok_k = self.compare(f"{d.name} K rows of position {p} (fork)", self.rows32(d.snap, "k")[:, p], d.ref.kc.a[:, p])
                ok_v = self.compare(f"{d.name} V rows of position {p} (fork)", self.rows32(d.snap, "v")[:, p], d.ref.vc.a[:, p])
                hurt = hurt or not (ok_k and ok_v)
            if hurt:
                self.heal_rows(d, 0, keep)
        if dkind != "kv8":
            return True
        if skind == "f32":   # the shadow takes the same fork from the same source
            self.gpu.runstate_fork(d.shadow, s.rs, n_pos)
            d.spairs, d.swk = d.pairs(), d.wk
        elif s.exact and any(t != 0 for t in d.tags):   # rows of a quantizing fork, handed on: between the shadows
            self.exact_tier(s)
            self.gpu.runstate_fork(d.shadow, s.shadow, keep)
            d.spairs, d.swk = d.pairs(), d.wk
        self.exact_tier(d)
        if not np.array_equal(d.snap["z"], s.snap["z"]):
            self.fail(f"{d.name}: its logits are not {s.name}'s after the fork")
        return True

    def op_fork_88(self):
        return self.op_fork("kv8", "kv8")

    def op_fork_832(self):
        return self.op_fork("kv8", "f32")

    def op_fork_3232(self):
        return self.op_fork("f32", "f32")

    # ---- state operations ----------------------------------------------------------------------------------------------
    def op_recreate(self):
        """the runstate is closed and made again, of either kind"""
        q, = self.pick()
        kind = ("kv8", "f32")[int(self.rng.random() < (0.25 if q.kind == "kv8" else 0.6))]
        n8 = sum(x.kind == "kv8" for x in self.main() if x is not q)
        if kind == "f32" and n8 < 3 or kind == "kv8" and n8 > N_SEQ - 3:   # (both kinds keep sources and destinations)
            kind = ("kv8", "f32")[kind == "kv8"]
        self.cur.update(seq=q.name, kind=kind)
        q.rs.close()
        self.make(q, q.wk, kind)
        self.settle({q: None})

    def op_reweight(self):
        """a sequence starts over at position 0 on the other weights object, with a prompt pass"""
        q, = self.pick()
        want = "ab"[q.wk == "a"]
        self.n_reweight += 1
        self.cur.update(seq=q.name, to=want)
        self.bind(q, want)
        q.zref, q.next_tok = None, None
        n = int(self.rng.integers(2, self.L // 3 + 1))
        (self.op_prefill_kv8 if q.kind == "kv8" else self.op_prefill_q8)(q, n, 0)

    def op_logits_only(self, kind):
        if kind != "write_logits":
            return super().op_logits_only(kind)
        q, = self.pick()
        z = self.rng.standard_normal(self.V).astype(f32)
        self.cur.update(seq=q.name)
        q.rs.write_logits(z)
        self.settle({q: (0, 0)})
        if not np.array_equal(q.snap["z"], bits(z)):
            self.fail(f"{q.name}: l2z_logits_read does not give the bits l2z_runstate_write_logits was handed")
        q.zref, q.next_tok = z.astype(np.float64), None
        return True

    def op_refusal(self):
        """one kind of refusal, at every call REFUSED_CALLS names for it: each returns its code and no bit moves"""
        if not self.refusal_queue:
            self.refusal_queue = [REFUSALS[i] for i in self.rng.permutation(len(REFUSALS))]
        kind = self.refusal_queue.pop()
        g, L, V, B = self.gpu, self.L, self.V, self.W.B
        kv = [x for x in self.main() if x.kind == "kv8"]
        pl = [x for x in self.main() if x.kind == "f32"]
        q, q2, f = kv[int(self.rng.integers(0, len(kv)))], self.seqs[N_SEQ], pl[int(self.rng.integers(0, len(pl)))]
        w, w32, p = self.w(q), self.W.w32, self.paged
        t = np.array([1, 5, 7], np.int32)
        bad = [V, -1][self.st["refusals"]["bad_token"] % 2]
        tb = np.array([1, 5, bad], np.int32)
        many = [x.rs for x in self.seqs[N_SEQ: N_SEQ + WIDE_MAX + 1]]
        calls = {
            "kv8_entry": (ERR_INVALID, [lambda: q.rs.transformer(5, 0, w), lambda: q.rs.prefill(t, 0, w32), lambda: q.rs.prefill_q8(t, 0, w),
                                        lambda: g.transformer_batch_q8([q.rs, q2.rs], [1, 1], [0, 0], w), lambda: q.rs.verify_q8(t, 0, w),
                                        lambda: g.transformer_wide([q.rs, q2.rs], [1, 1], [0, 0], w32),
                                        lambda: g.step_mixed([q.rs, q2.rs], [t, t[:1]], [0, 0], w32), lambda: q.rs.score(t, 0, w32)]),
            "mixed_kind": (ERR_INVALID, [lambda: g.transformer_wide_q8([q.rs, f.rs], [1, 1], [0, 0], w)]),
            "fork_kinds": (ERR_INVALID, [lambda: g.runstate_fork(f.rs, q.rs, 3), lambda: g.runstate_fork(p, q.rs, 3),
                                         lambda: g.runstate_fork(q.rs, p, 0)]),
            "prefill_kv8_wrong": (ERR_INVALID, [lambda: f.rs.prefill_kv8(t, 0, w), lambda: p.prefill_kv8(t, 0, w),
                                                lambda: q.rs.prefill_kv8(t, 0, w32)]),
            "past_end": (ERR_STATE, [lambda: q.rs.prefill_kv8(t, L - 2, w), lambda: g.transformer_wide_q8([q.rs, q2.rs], [5, 1], [L, 0], w)]),
            "bad_token": (ERR_STATE, [lambda: q.rs.prefill_kv8(tb, 0, w), lambda: g.transformer_wide_q8([q.rs, q2.rs], [bad, 1], [0, 0], w)]),
            "duplicate": (ERR_INVALID, [lambda: g.transformer_wide_q8([q.rs, q2.rs, q.rs], [1] * 3, [0] * 3, w)]),
            "rows129": (ERR_INVALID, [lambda: g.transformer_wide_q8(many, [1] * len(many), [0] * len(many), w)]),
        }
        code, fns = calls[kind]
        assert len(fns) == len(REFUSED_CALLS[kind]) and len(many) == WIDE_MAX + 1 and B is not None
        self.cur.update(seq=q.name)
        for name, fn in zip(REFUSED_CALLS[kind], fns):
            self.refused(kind, code, fn, note=name)

    # ---- the walk ------------------------------------------------------------------------------------------------------
    def schedule_kinds(self):
        """a warm-up of prompt passes, then every kind twice, one refusal of every kind and the rest by the weights of MAIN"""
        n_main = max(int(round(self.n_ops / 1.3)), 1)
        names = [k for k, _ in self.MAIN]
        weights = np.array([v for _, v in self.MAIN], np.float64)
        warm = ["prefill_kv8"] * 5 + ["prefill_q8"] * 2
        body = names * 2 + ["refusal"] * len(REFUSALS)
        fill = n_main - len(warm) - len(body)
        if fill > 0:
            body += [names[i] for i in self.rng.choice(len(names), fill, p=weights / weights.sum())]
        body = [body[i] for i in self.rng.permutation(len(body))]
        return (warm + body)[:n_main]

    def finish(self):
        """every carrier's rows below its depth against its reference's and its shadow's; then everything closes"""
        self.cur = dict(i=len(self.log), op="end")
        self.log.append(self.cur)
        if self.stop_at is None:
            for q in self.main():
                K, V = self.rows32(q.snap, "k"), self.rows32(q.snap, "v")
                kc = q.ref.kc.a if q.kind == "kv8" else q.ref.kc
                vc = q.ref.vc.a if q.kind == "kv8" else q.ref.vc
                for p in range(len(q.hist)):
                    self.compare(f"{q.name} K rows of position {p} at the end", K[:, p], kc[:, p], end=True)
                    self.compare(f"{q.name} V rows of position {p} at the end", V[:, p], vc[:, p], end=True)
                if q.kind == "kv8":
                    self.exact_tier(q, end=True)
        self.close()

    def close(self):
        for q in self.seqs[:N_SEQ]:
            if q.shadow is not None:
                q.shadow.close()
                q.shadow = None
        super().close()


def run(world, seed, n_ops=N_OPS, log=None, stop_at=None):
    """One walk of n_ops operations; returns its statistics, raises WalkFailure.  stop_at=k: replay up to operation k"""
    return Walk8(world, seed, n_ops=n_ops, log=log, stop_at=stop_at).run()


schedule, counts = qm.schedule, qm.counts


def coverage(stats, world):
    """what a walk's statistics lack of what every walk of `world` (a World) is to hold, dry or live; [] when nothing is"""
    ops, cross = stats["ops"], stats["cross"]
    bad = [f"{k}: {ops[k]} times" for k in OP_KINDS if ops[k] < (1 if k in ("trim", "fork_3232") else 2)]
    bad += [f"no refusal of the kind {k} at {c}" for k in REFUSALS for c in REFUSED_CALLS[k] if (k, c) not in stats["refused_calls"]]
    bad += [f"no wide step of {N_CLASSES[i]} rows" for i in range(len(N_CLASSES)) if not stats["n_classes"][i]]
    bad += [f"no prefill_kv8 call of {ROW_CLASSES[i]} rows" for i in range(len(ROW_CLASSES)) if not stats["row_classes"][i]]
    bad += [f"no prefill_kv8 call across position {e}" for e in EDGES if ("prefill_kv8", e) not in cross]
    bad += [f"no {what}" for what, key in (
        ("prefill_kv8 call that continues at a position that is no multiple of 64", "cont_off64"),
        ("prefill_kv8 call that ends exactly at seq_len", "end_at_len"), ("wide step that writes row seq_len - 1", "wide_last_row"),
        ("wide step with a carrier at position 0 beside one at 128 or deeper", "zero_beside_deep")) if not stats[key]]
    if stats["want_next"] != {False, True}:
        bad.append("wide steps not both with and without want_next")
    bad += [f"no {k} onto a destination with rows of its own beyond n_pos" for k in ("fork_88", "fork_832", "fork_3232")
            if k not in stats["fork_stale"]]
    bad += [f"no fork with n_pos {r} the source's depth" for r in ("below", "at", "above") if r not in stats["fork_rel"]]
    if world.name == "hs64" and world.pf_chunk == 0:
        if not stats["tail_after_flash"]:
            bad.append("no row-form chunk of at most 32 rows right behind a matrix-core chunk on the same runstate")
        if not stats["flash_high"]:
            bad.append("no matrix-core chunk that starts above position 64")
    if world.name == "kv24-v8k" and not stats["wide17"]:
        bad.append("no wide step of more than 16 rows (the register-blocked classifier)")
    if world.pf_chunk > 0 and (stats["chunks_max"] < 2 or stats["exact_skipped"]):
        bad.append("a chunked walk: no prompt of several chunks, or the exact tier was not held throughout")
    return bad
