"""The session walk's twin for the int8 group-quantized family: a seeded random walk over every way the q8
entry points move a sequence, each call on runstates that the OTHER entry points have already moved, held to a float64
reference (tests/ref_q8.py, mode "f64").  No GPU in this module: tests/test_q8_session_walk_cpu.py runs the walks dry --
ref_q8's "f32" mode stands in the device's place (DryGpu), so every check below runs there too --,
tests/test_gpu_q8_session_walk.py runs them on the device.

World: one f32 blob per shape and TWO weights objects made from it, "a" and "b" (g64: group size 32 and 64 of the same blob;
kv24 and kv24-flat: dim 96 is no multiple of 64, so "b" is group size 32 of the blob of the next seed); 8 runstates that carry
the sequences and 12 more that only serve as rows of the batched step (16 rows of one weights object need as many runstates),
all contiguous; live, f32 weights and a paged runstate for the refusals.

Per runstate the model holds
    wk      the weights object it is bound to; a call with the other one starts the sequence over at position 0 (re-weight)
    hist    the tokens it has consumed: KV rows below len(hist) are the sequence's
    ref     one ref_q8.Q8Model(mode="f64") fed exactly those tokens (a fork copies kc / vc rows, nothing is replayed)
    zref    the reference logits that belong to the runstate's logits (None: never written)
    vrows   the bits of the logits matrix of its last verify_q8 call
    snap    the last bit-snapshot of its logits and caches

The schedule -- which call, which runstates, row counts, positions, temperatures, coins -- is drawn from
np.random.default_rng([seed, ...]) and never looks at device output; only the ids the calls emit (and with them the accepted
counts) follow the device.

After every call:
    value      every logits row the call left (the runstate's, every verify row) and every K / V row it wrote against the
               reference: a row meets q8_cases.parity_ok, or it is an EXCEPTION (a quantized activation on the other side of
               a rounding boundary) and stays under q8_cases.LOOSE of its scale.  After an exception in the K / V rows of
               position p the reference takes the device's K / V rows of p (HEAL), so later rows are compared from the same
               state -- the fallback rule, Walk(heal=True); the rule in force is the plain one (heal=False): later rows are
               compared as they are.  The walk's share of exceptions is capped by the tests
    ids        every id whose row can be read is first_max of the row the device left for it, bit for bit, and the reference's
               argmax where the row is no exception and the reference's top-2 margin exceeds twice the parity bar; a greedy id
               from inside a loop call or a speculate_q8 loop (no row left) is the reference's argmax wherever the margin exceeds
               the loose bar (ident_blind); sampled ids are sample_batch's on the row; accepted counts are accept(tokens,
               out_next)
    footprint  bit for bit: an absent runstate (the spare and the paged one included) keeps logits and every cache row, a
               present one every row outside the call's positions; every runstate's verify rows stay what they were (l2z_verify_logits_read: rows of THIS runstate's
               last verify call), the row behind them and every row of a runstate that never verified are refused
At the end: every row below every sequence's depth against its reference; everything closes.
"""
import time
from collections import Counter

import numpy as np

import q8_batch_cases as bc
import q8_cases
import ref_q8
from session_model import WalkFailure, accept, bits, first_max, host_sampler, host_token

N_SEQ, N_FILL = 8, 12
BATCH_MAX = 16
SEG = 64
OK, ERR_INVALID, ERR_STATE = 0, -1, -6
EDGES = (64, 128)
SHAPES = {"kv24": bc.KV24, "g64": (128, 384, 2, 4, 2, 512, 160, 64), "kv24-flat": bc.KV24}
TEMPS = (0.4, 1.0)
TOP_PS = (0.0, 0.5, 0.9, 1.0)
REFUSALS = ("q8_to_f32", "f32_to_q8", "paged", "past_end", "bad_token", "duplicate", "rows17")
Q8_ENTRIES = ("prefill_q8", "transformer_batch_q8", "verify_q8")
REFUSED_CALLS = {   # the entry points every refusal of a kind is made at
    "q8_to_f32": ("prefill", "score", "transformer_batch", "verify", "prefill_batch", "transformer_wide"),
    "f32_to_q8": Q8_ENTRIES, "paged": Q8_ENTRIES, "past_end": Q8_ENTRIES + ("transformer",), "bad_token": Q8_ENTRIES,
    "duplicate": ("transformer_batch_q8",), "rows17": ("transformer_batch_q8", "verify_q8")}
OP_KINDS = ("transformer", "prefill_q8", "transformer_batch_q8", "verify_q8", "verify_q8_sampled", "greedy_run", "sample_run",
            "argmax", "argmax_batch", "sample_batch", "probs", "logits", "fork", "trim", "rewind", "recreate", "reweight")
PROBS_RTOL = 1e-5   # l2z_probs_read against the float64 softmax of the SAME device logits: f32 exp and sum of <= 512 terms


class DryError(RuntimeError):
    def __init__(self, code):
        super().__init__(f"code {code}")
        self.code = code


class DryWeights:
    def __init__(self, cfg, t, gs):
        self.cfg, self.t, self.gs = cfg, t, gs

    def close(self):
        pass


class DryState:
    """a runstate of the dry device: ref_q8's f32 mode behind RunState's methods"""

    def __init__(self, gpu, cfg):
        self.gpu, self.cfg = gpu, cfg
        self.kc = np.zeros((cfg.n_layers, cfg.seq_len, cfg.kv_dim), np.float32)
        self.vc = np.zeros_like(self.kc)
        self.z = np.zeros(cfg.vocab_size, np.float32)
        self.vz, self.models, self.loop = [], {}, None

    def model(self, w):
        if id(w) not in self.models:
            m = ref_q8.Q8Model(self.cfg, w.t, w.gs, "f32")
            m.kc, m.vc = self.kc, self.vc
            self.models[id(w)] = m
        return self.models[id(w)]

    def transformer(self, token, pos, w):
        self.z = self.model(w).transformer(int(token), int(pos)).astype(np.float32)

    def prefill_q8(self, tokens, pos0, w):
        for i, t in enumerate(tokens):
            self.transformer(t, pos0 + i, w)

    def verify_q8(self, tokens, pos0, w, temperature=0.0, top_p=1.0, coins=None):
        self.vz = []
        for i, t in enumerate(tokens):
            self.transformer(t, pos0 + i, w)
            self.vz.append(self.z)
        nxt = np.array([self.gpu.draw(z, temperature, top_p, 0.0 if coins is None else float(coins[i]))
                        for i, z in enumerate(self.vz)], np.int32)
        a = accept(tokens, nxt)
        self.z = self.vz[a]
        return nxt, a

    def verify_logits(self, row):
        if not 0 <= row < len(self.vz):
            raise DryError(ERR_STATE)
        return self.vz[row].copy()

    def greedy_begin(self, prompt=()):
        self.loop = dict(prompt=[int(t) for t in prompt], pos=0, tok=1, done=False)

    def sample_run(self, w, n_steps, temperature, top_p, coins=None):
        g, out = self.loop, []
        for i in range(n_steps):
            if g["done"] or g["pos"] >= self.cfg.seq_len:
                break
            self.transformer(g["tok"], g["pos"], w)
            if g["pos"] < len(g["prompt"]):
                nxt = g["prompt"][g["pos"]]
            else:
                nxt = self.gpu.draw(self.z, temperature, top_p, 0.0 if coins is None else float(coins[i]))
            out.append(nxt)
            g["tok"], g["pos"], g["done"] = nxt, g["pos"] + 1, nxt == 1
        return np.array(out, np.int32)

    def greedy_run(self, w, n_steps):
        return self.sample_run(w, n_steps, 0.0, 1.0)

    def argmax(self):
        return first_max(self.z)

    def logits(self):
        return self.z.copy()

    def probs(self, temperature=1.0):
        return self.gpu.softmax(self.z, temperature)

    def write_logits(self, z):
        self.z = np.array(z, np.float32)

    def read(self, name, offset, count):
        return (self.kc if name == "key_cache" else self.vc).reshape(-1)[offset:offset + count].copy()

    def close(self):
        pass


class DryGpu:
    """the binding's surface the walk uses, on DryStates"""
    L2ZError = DryError

    def __init__(self, H):
        self.H = H

    def RunState(self, cfg):
        return DryState(self, cfg)

    def softmax(self, z, temp):
        x = (z / np.float32(temp)).astype(np.float32)
        p = np.exp(x - x.max()).astype(np.float32)
        return (p / p.sum(dtype=np.float32)).astype(np.float32)

    def draw(self, z, temp, top_p, coin):
        return first_max(z) if temp == 0 else host_token(self.H, self.softmax(z, temp), top_p, coin)

    def transformer_batch_q8(self, states, tokens, pos, w):
        for s, t, p in zip(states, tokens, pos):
            s.transformer(t, p, w)

    def argmax_batch(self, states):
        return np.array([s.argmax() for s in states], np.int32)

    def sample_batch(self, states, temperature, top_p, coins):
        n = len(states)
        per = lambda v: [float(v)] * n if np.isscalar(v) else [float(x) for x in v]   # noqa: E731
        return np.array([self.draw(s.z, t, p, c) for s, t, p, c in zip(states, per(temperature), per(top_p), per(coins))], np.int32)

    def runstate_fork(self, dst, src, n_pos):
        dst.kc[:, :n_pos], dst.vc[:, :n_pos], dst.z = src.kc[:, :n_pos], src.vc[:, :n_pos], src.z.copy()


class World:
    """what the walks of one shape share; gpu=None: a dry world (ref_q8's f32 mode in the device's place)"""

    def __init__(self, pkg, name, gpu=None):
        ck = pkg.checkpoint
        self.name, self.live, self.B = name, gpu is not None, pkg.binding
        shp = SHAPES[name]
        self.cfg = ck.Config(*shp[:7])
        self.H = host_sampler()
        self.gpu = gpu if gpu is not None else DryGpu(self.H)
        if name == "kv24":
            self.shared = True
            blobs = {"a": bc.model("kv24")[2], "b": ck.synth_blob(self.cfg, True, bc.KV24_SEED + 1)}
            self.gs = {"a": 32, "b": 32}
        elif name == "kv24-flat":
            import hard_models
            self.shared = False
            blobs = {k: hard_models.hard_blob(ck, self.cfg, bc.KV24_SEED + i, "flat") for i, k in enumerate("ab")}
            self.gs = {"a": 32, "b": 32}
        else:
            self.shared = True
            blob = ck.synth_blob(self.cfg, True, 11)
            blobs = {"a": blob, "b": blob}
            self.gs = {"a": 32, "b": 64}
        self.blob = blobs["a"]
        self.body = {k: ck.v2_body_from_f32(self.cfg, blobs[k], self.shared, self.gs[k]) for k in "ab"}
        self.t = {k: ck.v2_carve(self.cfg, self.body[k], self.shared, self.gs[k]) for k in "ab"}
        if self.live:
            self.w = {k: gpu.Weights.from_q8(self.cfg, self.body[k], self.shared, self.gs[k]) for k in "ab"}
            self.w32 = gpu.Weights(self.cfg, self.blob, self.shared)
        else:
            self.w = {k: DryWeights(self.cfg, self.t[k], self.gs[k]) for k in "ab"}
            self.w32 = None

    def close(self):
        for w in list(self.w.values()) + [self.w32]:
            if w is not None:
                w.close()
        self.w, self.w32 = {}, None


class Seq:
    def __init__(self, idx):
        self.idx, self.name, self.fill = idx, ("s" if idx < N_SEQ else "x") + str(idx), idx >= N_SEQ
        self.rs = self.ref = self.wk = None
        self.reset()

    def reset(self):
        self.hist, self.zref, self.next_tok, self.snap, self.vrows, self.longest = [], None, None, None, [], 0


class Walk:
    def __init__(self, world, seed, n_ops=120, log=None, stop_at=None, heal=False):
        self.heal = heal
        self.W, self.seed, self.n_ops, self.say, self.stop_at = world, seed, n_ops, log, stop_at
        self.cfg, self.gpu, self.live = world.cfg, world.gpu, world.live
        self.V, self.L, self.kvd = self.cfg.vocab_size, self.cfg.seq_len, self.cfg.kv_dim
        self.rng = np.random.default_rng([int(seed), 0x5E58])
        self.seqs = [Seq(i) for i in range(N_SEQ + N_FILL)]
        self.spare = self.pool = self.paged = None
        self.others = []   # the spare and (live) the paged runstate: no call of the walk may move them
        self.log, self.failures, self.first_bad, self.cur = [], [], None, None
        self.n_reweight, self.refusal_queue = 0, []
        self.st = dict(ops=Counter(), refusals=Counter(), calls=0, rows=0, exceptions=0, worst=0.0, worst_at="", id_total=0,
                       id_under=0, id_exc=0, blind_total=0, blind_soft=0, end_rows=0, end_exceptions=0, cross=set(), batch_sides=0,
                       batch_rows=set(), reweight_prefill=set(), longer=0, fork_rel=set(), verify_temps=set(),
                       refused_calls=set())

    # ---- plumbing ----------------------------------------------------------------------------------------------------
    def fail(self, msg):
        self.failures.append((len(self.log) - 1, msg))
        if self.first_bad is None:
            self.first_bad = len(self.log) - 1
        if self.say:
            self.say(f"    FAIL {msg}")

    def make(self, q, wk):
        q.rs = self.gpu.RunState(self.cfg)
        q.reset()
        self.bind(q, wk)

    def bind(self, q, wk):
        q.wk, q.hist = wk, []
        q.ref = ref_q8.Q8Model(self.cfg, self.W.t[wk], self.W.gs[wk], "f64")

    def compare(self, what, got, ref, end=False):
        """the value rule on one row; True: the row meets the parity bar, False: an exception (or a failure)"""
        self.st["end_rows" if end else "rows"] += 1
        if q8_cases.parity_ok(got, ref):
            return True
        dev = q8_cases.scaled_dev(got, ref)
        self.st["end_exceptions" if end else "exceptions"] += 1
        self.cur["exceptions"] = self.cur.get("exceptions", 0) + 1
        if dev > self.st["worst"]:
            self.st["worst"], self.st["worst_at"] = dev, f"op {len(self.log) - 1} {what}"
        if not dev <= q8_cases.LOOSE:
            self.fail(f"{what}: {dev:.3e} of the scale off the reference, over the loose bar {q8_cases.LOOSE}")
        return False

    def feed(self, q, pos0, toks, zrows):
        """the reference consumes toks at pos0 ..; every K / V row the call wrote and the device's logits rows zrows
        {i: row} are compared as it goes, and an exception in the K / V rows of a position heals the reference there.
        Returns the reference's logits rows and whether each compared logits row met the parity bar"""
        K, V = q.snap[1].view(np.float32), q.snap[2].view(np.float32)
        zs, oks = [], {}
        for i, t in enumerate(toks):
            p = pos0 + i
            z = q.ref.transformer(int(t), p)
            ok_k = self.compare(f"{q.name} K rows of position {p}", K[:, p], q.ref.kc[:, p])
            ok_v = self.compare(f"{q.name} V rows of position {p}", V[:, p], q.ref.vc[:, p])
            if self.heal and not (ok_k and ok_v):
                q.ref.kc[:, p], q.ref.vc[:, p] = K[:, p], V[:, p]
            if i in zrows:
                oks[i] = self.compare(f"{q.name} logits of position {p}", zrows[i], z)
            zs.append(z)
        return zs, oks

    def bar(self, z):
        top = np.partition(z, -2)[-2:]
        return q8_cases.PARITY_ATOL + q8_cases.PARITY_RTOL * float(np.abs(top).max()), float(top[1] - top[0])

    def ident(self, what, got, z_dev, z_ref, row_ok):
        """an id taken at temperature 0 from the device row z_dev whose reference is z_ref"""
        if int(got) != first_max(z_dev):
            self.fail(f"{what}: id {int(got)} is not the first maximum {first_max(z_dev)} of the row the device left")
        self.st["id_total"] += 1
        bar, margin = self.bar(z_ref)
        if not row_ok:
            self.st["id_exc"] += 1
        elif margin > 2 * bar:
            if int(got) != first_max(z_ref):
                self.fail(f"{what}: id {int(got)}, the reference's argmax is {first_max(z_ref)} at margin {margin:.3e}")
        else:
            self.st["id_under"] += 1

    def ident_blind(self, what, got, z_ref):
        """an id taken at temperature 0 in mid-loop, from a row nobody can read: it is the reference's argmax wherever the
        top-2 margin exceeds the loose bar (what an exception row may be off); where the margin exceeds twice the parity bar
        only, another id can come from an exception row alone -- counted (blind_soft), and capped by the tests as the
        exceptions are"""
        self.st["blind_total"] += 1
        bar, margin = self.bar(z_ref)
        if int(got) == first_max(z_ref):
            return
        if margin > q8_cases.LOOSE * float(np.abs(z_ref).max()):
            self.fail(f"{what}: id {int(got)}, the reference's argmax is {first_max(z_ref)} at margin {margin:.3e}, over the loose bar")
        elif margin > 2 * bar:
            self.st["blind_soft"] += 1
        else:
            self.st["id_under"] += 1

    def drawn(self, what, got, z_dev, temp, top_p, coin):
        """a sampled id: l2z_sample_batch's on the same logits"""
        self.spare.write_logits(z_dev)
        self.others[0].snap[0] = bits(z_dev).copy()
        want = int(self.gpu.sample_batch([self.spare], temp, top_p, coin)[0])
        if int(got) != want:
            self.fail(f"{what}: id {int(got)}, l2z_sample_batch draws {want} from the same logits (t {temp} p {top_p} coin {coin})")

    def wrong(self, t):
        return (int(t) - 2 + 1) % (self.V - 2) + 2

    # ---- device state ------------------------------------------------------------------------------------------------
    def read(self, q):
        n, shape = self.cfg.n_layers * self.L * self.kvd, (self.cfg.n_layers, self.L, self.kvd)
        return [bits(q.rs.logits()), bits(q.rs.read("key_cache", 0, n)).reshape(shape).copy(),
                bits(q.rs.read("value_cache", 0, n)).reshape(shape).copy()]

    def settle(self, touched):
        """after a call: touched = {seq: (lo, hi) rows the call may write, or None: any row}: the footprint"""
        for q in self.seqs + self.others:
            new, old = self.read(q), q.snap
            if old is not None and not (q in touched and touched[q] is None):
                keep = np.ones(self.L, bool)
                if q in touched:
                    keep[touched[q][0]: touched[q][1]] = False
                for name, a, b in (("key", old[1], new[1]), ("value", old[2], new[2])):
                    if not np.array_equal(a[:, keep, :], b[:, keep, :]):
                        rows = np.flatnonzero(keep)[np.any(a[:, keep, :] != b[:, keep, :], axis=(0, 2))]
                        self.fail(f"{q.name}: {name} cache rows {rows[:8].tolist()} changed outside the call's range "
                                  f"{touched.get(q, 'absent')}")
                if q not in touched and not np.array_equal(old[0], new[0]):
                    self.fail(f"{q.name}: logits changed by a call it took no part in")
            q.snap = new
            # the verify rows are the runstate's own last verify call's, and nothing else is a row
            for i, row in enumerate(q.vrows):
                if not np.array_equal(bits(q.rs.verify_logits(i)), row):
                    self.fail(f"{q.name}: row {i} of its last verify call's logits changed")
            try:
                q.rs.verify_logits(len(q.vrows))
                self.fail(f"{q.name}: verify_logits_read answers for row {len(q.vrows)}, its last verify call had {len(q.vrows)} rows")
            except self.gpu.L2ZError as e:
                if e.code != ERR_STATE:
                    self.fail(f"{q.name}: verify_logits_read code {e.code}, expected {ERR_STATE}")

    def refused(self, kind, code, fn, note=""):
        self.st["refusals"][kind] += 1
        self.st["refused_calls"].add((kind, note))
        self.cur.update(refusal=kind, code=code)
        if self.live:
            try:
                fn()
                self.fail(f"{kind}: the call passed, expected code {code}")
            except self.gpu.L2ZError as e:
                if e.code != code:
                    self.fail(f"{kind}: code {e.code}, expected {code} ({e})")
        self.settle({})

    # ---- choosing ----------------------------------------------------------------------------------------------------
    def main(self):
        return self.seqs[:N_SEQ]

    def pick(self, n=1, pool=None):
        pool = self.main() if pool is None else pool
        return [pool[i] for i in self.rng.permutation(len(pool))[:n]]

    def pick_deep(self, room):
        """one sequence: every other time the deepest that still has `room` positions, so that some reach the upper segments"""
        q, = self.pick()
        have = [x for x in self.main() if len(x.hist) + room <= self.L]
        if self.rng.random() < 0.6 and have:
            q = max(have, key=lambda x: (len(x.hist), -x.idx))
        return q

    def plan(self, q, n, aim=True):
        """where q's next n rows go: on from its depth, now and then a rewind, and -- where the depth allows it -- often
        right across a segment edge; and the tokens it is fed there"""
        d = len(q.hist)
        pos0 = d
        u = self.rng.random()
        if d + n > self.L or u < 0.12:
            pos0 = int(self.rng.integers(0, max(min(d, self.L - n), 0) + 1))
        elif aim and n > 1 and u < 0.6:
            ok = [e for e in EDGES if max(e - n + 1, 0) <= min(d, e - 1, self.L - n)]
            if ok:
                e = ok[-1] if self.rng.random() < 0.7 else ok[0]
                pos0 = int(self.rng.integers(max(e - n + 1, 0), min(d, e - 1, self.L - n) + 1))
        toks = self.rng.integers(2, self.V, n).astype(np.int32)
        if pos0 == 0:
            toks[0] = 1
        elif pos0 == d and q.next_tok is not None and self.rng.random() < 0.7:
            toks[0] = q.next_tok
        if pos0 < d:
            self.cur["rewind"] = self.cur.get("rewind", 0) + 1
        return pos0, toks

    def crossed(self, kind, pos0, n):
        for e in EDGES:
            if pos0 < e <= pos0 + n - 1:
                self.st["cross"].add((kind, e))

    def after(self, q, pos0, toks, zs, keep):
        """q consumed toks[:keep] at pos0 ..; its logits are the reference row zs[keep - 1]'s"""
        q.hist = q.hist[:pos0] + [int(t) for t in toks[:keep]]
        q.zref = zs[keep - 1]

    def w(self, q):
        return self.W.w[q.wk]

    # ---- the calls that move one sequence --------------------------------------------------------------------------
    def op_transformer(self):
        q = self.pick_deep(1)
        pos0, t = self.plan(q, 1)
        self.cur.update(seq=q.name, pos=pos0, tok=int(t[0]))
        q.rs.transformer(int(t[0]), pos0, self.w(q))
        self.settle({q: (pos0, pos0 + 1)})
        zs, _ = self.feed(q, pos0, t, {0: q.snap[0].view(np.float32)})
        self.after(q, pos0, t, zs, 1)
        q.next_tok = None

    def op_prefill_q8(self, q=None, n=None, pos0=None):
        if q is None:
            n = int(self.rng.integers(1, self.L // 3 + 1))
            q = self.pick_deep(n)
            if self.rng.random() < 0.35:
                n = min(q.longest + int(self.rng.integers(1, 9)), self.L // 3)
            pos0, t = self.plan(q, n)
        else:
            t = np.append(1, self.rng.integers(2, self.V, n - 1)).astype(np.int32)
        self.cur.update(seq=q.name, pos=pos0, n=n)
        q.rs.prefill_q8(t, pos0, self.w(q))
        if q.longest and n > q.longest:
            self.st["longer"] += 1
        q.longest = max(q.longest, n)
        self.crossed("prefill_q8", pos0, n)
        self.settle({q: (pos0, pos0 + n)})
        zs, _ = self.feed(q, pos0, t, {n - 1: q.snap[0].view(np.float32)})
        self.after(q, pos0, t, zs, n)
        q.next_tok = None

    def op_transformer_batch_q8(self):
        wk = "ab"[int(self.rng.integers(0, 2))]
        k = self.st["ops"]["transformer_batch_q8"]   # (the first call has 16 rows, the second one)
        n = (BATCH_MAX, 1)[k] if k < 2 else int(self.rng.integers(1, BATCH_MAX + 1))
        if n > sum(q.wk == wk for q in self.main()) + N_FILL:   # (the object that more sequences are bound to: at least 4)
            wk = "ab"[wk == "a"]
        mains = [q for q in self.main() if q.wk == wk]
        mains = [mains[i] for i in self.rng.permutation(len(mains))]
        if self.rng.random() < 0.8:   # the deepest and the shallowest first: rows on both sides of a segment edge
            mains.sort(key=lambda x: len(x.hist))
            mains = mains[-1:] + mains[:-1]
        m = int(self.rng.integers(0, len(mains) + 1))
        qs = mains[: min(max(m, n - N_FILL), n, len(mains))]
        fills = self.pick(n - len(qs), self.seqs[N_SEQ:])
        for f in fills:   # a row runstate that last ran on the other object starts over
            if f.wk != wk:
                self.bind(f, wk)
        qs = qs + fills
        qs = [qs[i] for i in self.rng.permutation(len(qs))]
        plans = [self.plan(q, 1, aim=False) for q in qs]
        pos, tok = [p for p, _ in plans], [int(t[0]) for _, t in plans]
        self.cur.update(seqs=[q.name for q in qs], pos=pos, wk=wk)
        self.gpu.transformer_batch_q8([q.rs for q in qs], tok, pos, self.W.w[wk])
        self.st["batch_rows"].add(len(qs))
        if any(p < SEG for p in pos) and any(p >= SEG for p in pos):
            self.st["batch_sides"] += 1
        self.settle({q: (p, p + 1) for q, p in zip(qs, pos)})
        for q, p, t in zip(qs, pos, tok):
            zs, _ = self.feed(q, p, [t], {0: q.snap[0].view(np.float32)})
            self.after(q, p, [t], zs, 1)
            q.next_tok = None

    def op_verify_q8(self, sampled=False):
        n = int(self.rng.integers(1, BATCH_MAX + 1))
        q = self.pick_deep(n)
        pos0, t0 = self.plan(q, n)
        temp = float(self.rng.choice(TEMPS)) if sampled else 0.0
        top_p = float(self.rng.choice(TOP_PS)) if sampled else 1.0
        coins = self.rng.random(n, dtype=np.float32)
        a_plan = int(self.rng.integers(0, n))
        # the draft: the reference's greedy continuation behind t0, guess a_plan made wrong
        toks, tok = [int(t0[0])], int(t0[0])
        for i in range(n - 1):
            tok = first_max(q.ref.transformer(tok, pos0 + i))
            toks.append(tok)
        if a_plan < n - 1:
            toks[a_plan + 1] = self.wrong(toks[a_plan + 1])
        self.cur.update(seq=q.name, pos=pos0, n=n, temp=temp, top_p=top_p)
        nxt, a = q.rs.verify_q8(toks, pos0, self.w(q), temp, top_p, coins if sampled else None)
        q.vrows = [bits(q.rs.verify_logits(i)).copy() for i in range(n)]
        self.st["verify_temps"].add(sampled)
        self.crossed("verify_q8", pos0, n)
        self.settle({q: (pos0, pos0 + n)})
        zd = [r.view(np.float32) for r in q.vrows]
        zs, oks = self.feed(q, pos0, toks, dict(enumerate(zd)))
        for i in range(n):
            if sampled:
                self.drawn(f"{q.name} verify row {i}", nxt[i], zd[i], temp, top_p, float(coins[i]))
            else:
                self.ident(f"{q.name} verify row {i}", nxt[i], zd[i], zs[i], oks[i])
        if a != accept(toks, nxt):
            self.fail(f"{q.name}: accepted {a}, the verdict rule gives {accept(toks, nxt)} on {list(nxt)}")
        a = accept(toks, nxt)
        if not np.array_equal(q.snap[0], q.vrows[a]):
            self.fail(f"{q.name}: its logits are not row {a} of the verify call, the last accepted one")
        self.cur["accepted"] = int(a)
        self.after(q, pos0, toks, zs, a + 1)
        q.next_tok = int(nxt[a])

    def op_verify_q8_sampled(self):
        self.op_verify_q8(sampled=True)

    def op_greedy_run(self, sampled=False):
        """greedy_begin, then two loop calls: the second goes on in mid-sequence"""
        q, = self.pick()
        prompt = self.rng.integers(2, self.V, int(self.rng.choice([0, 1, 3, 6]))).tolist()
        parts = [int(self.rng.integers(3, 13)), int(self.rng.integers(1, 9))]
        temp = float(self.rng.choice(TEMPS)) if sampled else 0.0
        top_p = float(self.rng.choice(TOP_PS)) if sampled else 1.0
        self.cur.update(seq=q.name, pos=0, n=sum(parts), parts=parts, begin=prompt, temp=temp, top_p=top_p)
        q.rs.greedy_begin(prompt)
        pos, tok = 0, 1
        for want in parts:
            coins = self.rng.random(want, dtype=np.float32)
            if tok == 1 and pos > 0:
                break   # the loop ended on a BOS
            out = q.rs.sample_run(self.w(q), want, temp, top_p, coins) if sampled else q.rs.greedy_run(self.w(q), want)
            out = [int(t) for t in out]
            end = out.index(1) + 1 if 1 in out else want
            if len(out) != end:
                self.fail(f"{q.name}: the loop produced {len(out)} ids, expected {end}")
                break
            fed = [tok] + out[:-1]
            # (the device looks for a BOS once a chunk of 64 steps: the steps behind one have run, so after a BOS the call's
            # whole range may be written and the header does not say which step's logits the runstate holds)
            bos = out[-1] == 1
            self.settle({q: (pos, min(pos + want, self.L))})
            z_dev = q.snap[0].view(np.float32)
            zs, oks = self.feed(q, pos, fed, {} if bos else {len(fed) - 1: z_dev})
            self.cur.setdefault("spans", []).append((pos, pos + len(out)))   # the positions the call really stepped
            for i, t in enumerate(out):
                if pos + i < len(prompt):
                    if t != prompt[pos + i]:
                        self.fail(f"{q.name}: step at prompt position {pos + i} gave {t}, the prompt holds {prompt[pos + i]}")
                elif not sampled and (i < len(out) - 1 or bos):   # an id of mid-call: its row is gone
                    self.ident_blind(f"{q.name} loop id {i}", t, zs[i])
            if pos + len(out) - 1 >= len(prompt) and not bos:   # the last id comes from the logits the call left
                if sampled:
                    self.drawn(f"{q.name} loop's last id", out[-1], z_dev, temp, top_p, float(coins[len(out) - 1]))
                else:
                    self.ident(f"{q.name} loop's last id", out[-1], z_dev, zs[-1], oks[len(fed) - 1])
            self.after(q, pos, fed, zs, len(fed))
            if bos:
                q.zref = None
            pos, tok = pos + len(out), out[-1]
        q.next_tok = tok

    def op_sample_run(self):
        self.op_greedy_run(sampled=True)

    def op_speculate_q8(self):
        """binding.speculate_q8, greedy: prefill_q8 of BOS + prompt, argmax, verify_q8 rounds; the draft is the reference's
        own greedy continuation with every third guess made wrong"""
        q, = self.pick()
        prompt = self.rng.integers(2, self.V, 3).tolist()
        steps, k = int(self.rng.integers(10, 21)), int(self.rng.integers(2, 6))
        spoil = self.rng.random(steps + k + 1) < 0.3
        self.cur.update(seq=q.name, pos=0, n=steps, k=k, begin=prompt)
        cont, tok = list(prompt), 1
        for p in range(steps + k):   # (the reference's rows are written again below, from the tokens the device consumed)
            z = q.ref.transformer(tok, p)
            if p >= len(prompt):
                cont.append(first_max(z))
            tok = cont[p]

        def drafter(hist, kk):
            at = len(hist) - 1
            return [self.wrong(t) if spoil[at + j] else t for j, t in enumerate(cont[at: at + kk])]
        ids, stats = self.W.B.speculate_q8(q.rs, self.w(q), prompt, steps, k, drafter)
        ids = [int(t) for t in ids]
        self.cur.update(accepted=stats["accepted"], offered=stats["offered"])
        q.vrows = []
        i = 0
        while True:   # (the rows of the loop's last verify call, however many they were)
            try:
                q.vrows.append(bits(q.rs.verify_logits(i)).copy())
                i += 1
            except self.gpu.L2ZError:
                break
        self.settle({q: (0, min(steps + k, self.L))})
        fed = [1] + ids[:-1]
        whole = 1 not in ids and len(ids) == steps
        z_dev = q.snap[0].view(np.float32)
        zs, oks = self.feed(q, 0, fed, {len(fed) - 1: z_dev} if whole else {})
        if ids[: len(prompt)] != prompt[: len(ids)]:
            self.fail(f"{q.name}: speculate_q8 does not echo the prompt: {ids[:len(prompt)]}")
        for i in range(len(prompt), len(ids) - whole):   # the ids behind the prompt whose rows are gone
            self.ident_blind(f"{q.name} speculate_q8 id {i}", ids[i], zs[i])
        if whole:
            self.ident(f"{q.name} speculate_q8's last id", ids[-1], z_dev, zs[-1], oks[len(fed) - 1])
        self.after(q, 0, fed, zs, len(fed))
        if not whole:
            q.zref = None   # a BOS in mid-round: the header does not say which row's logits the runstate holds
        q.next_tok = ids[-1]

    # ---- logits-only calls -----------------------------------------------------------------------------------------
    def op_logits_only(self, kind):
        have = [q for q in self.seqs if q.zref is not None]
        if not have:
            return False
        if kind in ("argmax", "probs", "logits"):
            q = have[int(self.rng.integers(0, len(have)))]
            self.cur.update(seq=q.name)
            z_dev = q.rs.logits()
            ok = q8_cases.parity_ok(z_dev, q.zref)
            if kind == "argmax":
                self.ident(f"{q.name} argmax", q.rs.argmax(), z_dev, q.zref, ok)
            elif kind == "logits":
                if not np.array_equal(bits(z_dev), q.snap[0]):
                    self.fail(f"{q.name}: l2z_logits_read gives other bits than right after the call that wrote them")
            else:
                temp = float(self.rng.choice(TEMPS))
                self.cur.update(temp=temp)
                x = z_dev.astype(np.float64) / temp
                p = np.exp(x - x.max())
                p /= p.sum()
                err = float(np.abs(q.rs.probs(temp).astype(np.float64) - p).max())
                if not err <= PROBS_RTOL * float(p.max()):
                    self.fail(f"{q.name}: probs {err:.3e} off the float64 softmax of its own logits, bar {PROBS_RTOL * float(p.max()):.3e}")
        else:
            qs = [have[i] for i in self.rng.permutation(len(have))[: int(self.rng.integers(1, min(len(have), BATCH_MAX) + 1))]]
            self.cur.update(seqs=[q.name for q in qs])
            zd = [q.rs.logits() for q in qs]
            if kind == "argmax_batch":
                for q, t, z in zip(qs, self.gpu.argmax_batch([q.rs for q in qs]), zd):
                    self.ident(f"{q.name} argmax_batch", t, z, q.zref, q8_cases.parity_ok(z, q.zref))
            else:
                temp = [float(self.rng.choice((0.0,) + TEMPS)) for _ in qs]
                top_p = [float(self.rng.choice(TOP_PS)) for _ in qs]
                coins = self.rng.random(len(qs), dtype=np.float32)
                self.cur.update(temp=temp, top_p=top_p)
                got = self.gpu.sample_batch([q.rs for q in qs], temp, top_p, coins)
                for q, t, tj, pj, cj, z in zip(qs, got, temp, top_p, coins, zd):
                    if tj == 0:
                        self.ident(f"{q.name} sample_batch", t, z, q.zref, q8_cases.parity_ok(z, q.zref))
                    else:   # the header's own statement: the host sampler's walk on l2z_probs_read's probabilities
                        want = host_token(self.W.H, q.rs.probs(tj), pj, float(cj))
                        if int(t) != want:
                            self.fail(f"{q.name}: sample_batch {int(t)}, the host sampler draws {want} (t {tj} p {pj} coin {cj})")
        self.settle({})
        return True

    # ---- state operations ------------------------------------------------------------------------------------------
    def op_fork(self):
        src = [q for q in self.main() if q.zref is not None]
        if not src:
            return False
        s = src[int(self.rng.integers(0, len(src)))]
        dsts = [q for q in self.main() if q is not s and q.wk == s.wk]
        if not dsts:
            return False
        d = dsts[int(self.rng.integers(0, len(dsts)))]
        depth = len(s.hist)
        rel = ("below", "at", "above")[self.st["ops"]["fork"] % 3]
        if rel == "below" and depth == 0 or rel == "above" and depth == self.L:
            rel = "at"
        n_pos = {"below": int(self.rng.integers(0, max(depth, 1))), "at": depth,
                 "above": int(self.rng.integers(depth + 1, self.L + 1)) if depth < self.L else depth}[rel]
        self.cur.update(dst=d.name, src=s.name, n_pos=n_pos, rel=rel)
        self.gpu.runstate_fork(d.rs, s.rs, n_pos)
        self.st["fork_rel"].add(rel)
        keep = min(n_pos, depth)
        d.hist, d.zref, d.next_tok = s.hist[:keep], s.zref, None
        d.ref.kc[:, :keep], d.ref.vc[:, :keep] = s.ref.kc[:, :keep], s.ref.vc[:, :keep]
        self.settle({d: (0, n_pos)})
        if not np.array_equal(d.snap[0], s.snap[0]):
            self.fail(f"{d.name}: its logits are not {s.name}'s after the fork")
        for a, b in ((d.snap[1], s.snap[1]), (d.snap[2], s.snap[2])):
            if not np.array_equal(a[:, :n_pos, :], b[:, :n_pos, :]):
                self.fail(f"{d.name}: cache rows below {n_pos} are not {s.name}'s after the fork")
        return True

    def op_trim(self):
        """l2z_runstate_trim is the paged runstates' call: on a contiguous one it is refused and nothing moves"""
        q, = self.pick()
        n_pos = int(self.rng.integers(0, self.L + 1))
        self.cur.update(seq=q.name, n_pos=n_pos)
        if self.live:
            try:
                q.rs.trim(n_pos)
                self.fail(f"{q.name}: l2z_runstate_trim passed on a contiguous runstate")
            except self.gpu.L2ZError as e:
                if e.code != ERR_INVALID:
                    self.fail(f"{q.name}: l2z_runstate_trim code {e.code}, expected {ERR_INVALID}")
        self.settle({})

    def op_recreate(self):
        q, = self.pick()
        self.cur.update(seq=q.name)
        q.rs.close()
        self.make(q, q.wk)
        self.settle({q: None})

    def op_reweight(self):
        """a sequence starts over at position 0 on the other weights object; two times in three with a prompt pass"""
        want = "ab"[self.n_reweight % 2]
        have = [q for q in self.main() if q.wk != want] or self.main()
        q = have[int(self.rng.integers(0, len(have)))]
        first = "prefill_q8" if self.n_reweight % 3 != 2 else "transformer"
        self.n_reweight += 1
        self.cur.update(seq=q.name, to=want, first=first)
        src = q.wk
        self.bind(q, want)
        q.zref, q.next_tok = None, None
        if first == "prefill_q8":
            self.op_prefill_q8(q, int(self.rng.integers(2, self.L // 3 + 1)), 0)
            if src != want:
                self.st["reweight_prefill"].add(src + want)
        else:
            q.rs.transformer(1, 0, self.w(q))
            self.settle({q: (0, 1)})
            zs, _ = self.feed(q, 0, [1], {0: q.snap[0].view(np.float32)})
            self.after(q, 0, [1], zs, 1)

    def op_refusal(self):
        """one kind of refusal, at every entry point REFUSED_CALLS names for it: each call returns its code and no bit moves"""
        if not self.refusal_queue:   # (every kind comes round before one comes twice)
            self.refusal_queue = [REFUSALS[i] for i in self.rng.permutation(len(REFUSALS))]
        kind = self.refusal_queue.pop()
        g, L, V = self.gpu, self.L, self.V
        q, = self.pick()
        w, w32, p = self.w(q), self.W.w32, self.paged
        rs = lambda qs: [x.rs for x in qs]   # noqa: E731
        t = np.array([1, 5, 7], np.int32)
        same = [x for x in self.seqs if x.wk == q.wk and x is not q][:2]
        n = 1 + len(same)
        bad = [V, -1][self.st["refusals"]["bad_token"] % 2]
        tb = np.array([1, 5, bad], np.int32)
        dup, many = [q] + same[:1] + [q], self.seqs[:BATCH_MAX + 1]
        calls = {
            "q8_to_f32": (ERR_INVALID, [lambda: q.rs.prefill(t, 0, w), lambda: q.rs.score(t, 0, w),
                                        lambda: g.transformer_batch(rs([q]), [1], [0], w), lambda: q.rs.verify(t, 0, w),
                                        lambda: g.prefill_batch(rs([q]), [t], [0], w), lambda: g.transformer_wide(rs([q]), [1], [0], w)]),
            "f32_to_q8": (ERR_INVALID, [lambda: q.rs.prefill_q8(t, 0, w32), lambda: g.transformer_batch_q8(rs([q]), [1], [0], w32),
                                        lambda: q.rs.verify_q8(t, 0, w32)]),
            "paged": (ERR_INVALID, [lambda: p.prefill_q8(t, 0, w), lambda: g.transformer_batch_q8([q.rs, p], [1, 1], [0, 0], w),
                                    lambda: p.verify_q8(t, 0, w)]),
            "past_end": (ERR_STATE, [lambda: q.rs.prefill_q8(t, L - 2, w),
                                     lambda: g.transformer_batch_q8(rs([q] + same), [5] * n, [L] + [0] * len(same), w),
                                     lambda: q.rs.verify_q8(t, L - 2, w), lambda: q.rs.transformer(5, L, w)]),
            "bad_token": (ERR_STATE, [lambda: q.rs.prefill_q8(tb, 0, w),
                                      lambda: g.transformer_batch_q8(rs([q] + same), [bad] + [1] * len(same), [0] * n, w),
                                      lambda: q.rs.verify_q8(tb, 0, w)]),
            "duplicate": (ERR_INVALID, [lambda: g.transformer_batch_q8(rs(dup), [1] * len(dup), [0] * len(dup), w)]),
            "rows17": (ERR_INVALID, [lambda: g.transformer_batch_q8(rs(many), [1] * 17, [0] * 17, w),
                                     lambda: q.rs.verify_q8([1] + [5] * 16, 0, w)]),
        }
        code, fns = calls[kind]
        assert len(fns) == len(REFUSED_CALLS[kind])
        self.cur.update(seq=q.name)
        for name, fn in zip(REFUSED_CALLS[kind], fns):
            self.refused(kind, code, fn, note=name)

    # ---- the walk ------------------------------------------------------------------------------------------------------
    MAIN = (("transformer", 5), ("prefill_q8", 9), ("transformer_batch_q8", 7), ("verify_q8", 7), ("verify_q8_sampled", 5),
            ("greedy_run", 4), ("sample_run", 4), ("fork", 7), ("trim", 3), ("recreate", 3), ("reweight", 5))
    AFTER = ("argmax", "argmax_batch", "sample_batch", "probs", "logits")

    def schedule_kinds(self):
        """a warm-up of prompt passes, then every kind three times (a re-weight four times), one loop of speculate_q8, one
        refusal in ten operations and the rest by the weights of MAIN, shuffled"""
        n_main = max(int(round(self.n_ops / 1.4)), 1)
        names = [k for k, _ in self.MAIN]
        weights = np.array([v for _, v in self.MAIN], np.float64)
        warm = ["prefill_q8"] * 8
        body = names * 3 + ["reweight", "speculate_q8"] + ["refusal"] * max(self.n_ops // 10, 1)
        fill = n_main - len(warm) - len(body)
        if fill > 0:
            body += [names[i] for i in self.rng.choice(len(names), fill, p=weights / weights.sum())]
        body = [body[i] for i in self.rng.permutation(len(body))]
        return (warm + body)[:n_main]

    def one(self, kind):
        self.cur = dict(i=len(self.log), op=kind)
        self.log.append(self.cur)
        self.st["calls"] += 1
        if kind in self.AFTER:
            done = self.op_logits_only(kind)
        else:
            done = getattr(self, "op_" + kind)()
        if done is False:
            self.cur["skipped"] = True
        elif "refusal" not in self.cur:
            self.st["ops"][kind] += 1
            if self.cur.get("rewind"):
                self.st["ops"]["rewind"] += 1
        if self.say:
            self.say(repr(self.cur))

    def run(self):
        t0 = time.perf_counter()
        plan = self.schedule_kinds()
        try:
            self.spare = self.gpu.RunState(self.cfg)
            if self.live:
                self.pool = self.gpu.KvPool(self.cfg, 2)
                self.paged = self.gpu.RunState(self.cfg, pool=self.pool)
            for q in self.seqs:
                self.make(q, "ab"[q.idx % 2])
            for name, rs in (("spare", self.spare), ("paged", self.paged)):
                if rs is not None:
                    o = Seq(-1)
                    o.name, o.rs = name, rs
                    self.others.append(o)
            self.cur = dict(i=-1, op="begin")
            self.settle({q: None for q in self.seqs + self.others})
            after = []
            follow = set(self.rng.choice(len(plan), min(max(self.n_ops - len(plan), 0), len(plan)), replace=False).tolist())
            for k, kind in enumerate(plan):
                if self.stop_at is not None and len(self.log) > self.stop_at:
                    break
                self.one(kind)
                if k in follow:
                    if not after:
                        after = [self.AFTER[i] for i in self.rng.permutation(len(self.AFTER))]
                    self.one(after.pop())
            self.finish()
        except WalkFailure:
            raise
        except Exception as e:   # a call the model expected to pass did not (or the walk itself broke): the state is unknown
            self.fail(f"{type(e).__name__}: {e}")
            self.close()
            raise WalkFailure(self.seed, self.first_bad, self.failures, self.log) from e
        st = self.st
        st["wall"], st["log"] = time.perf_counter() - t0, self.log
        st["exc_share"] = st["exceptions"] / max(st["rows"], 1)
        st["soft_share"] = st["blind_soft"] / max(st["blind_total"], 1)
        st["under_share"] = st["id_under"] / max(st["id_total"], 1)
        if self.failures:
            raise WalkFailure(self.seed, self.first_bad, self.failures, self.log)
        return st

    def finish(self):
        """every sequence's rows below its depth against its reference's; then everything closes"""
        self.cur = dict(i=len(self.log), op="end")
        self.log.append(self.cur)
        if self.stop_at is None:
            for q in self.seqs:
                d = len(q.hist)
                for p in range(d):   # (position by position, each at its own scale; counted apart from the walk's rows)
                    self.compare(f"{q.name} K rows of position {p} at the end", q.snap[1].view(np.float32)[:, p], q.ref.kc[:, p], end=True)
                    self.compare(f"{q.name} V rows of position {p} at the end", q.snap[2].view(np.float32)[:, p], q.ref.vc[:, p], end=True)
        self.close()

    def close(self):
        if not self.others:   # (closed before the snapshots were made)
            self.others = [o for o in (self.spare, self.paged) if o is not None]
        for q in self.seqs + self.others:
            rs = q.rs if isinstance(q, Seq) else q
            if rs is not None:
                rs.close()
            if isinstance(q, Seq):
                q.rs = None
        self.spare = self.paged = None
        self.others = []
        if self.pool is not None:
            self.pool.close()
            self.pool = None


def run(world, seed, n_ops=120, log=None, stop_at=None, heal=False):
    """One walk of n_ops operations; returns its statistics, raises WalkFailure.  stop_at=k: replay up to operation k;
    heal=True: the fallback exception rule (the module's docstring)"""
    return Walk(world, seed, n_ops=n_ops, log=log, stop_at=stop_at, heal=heal).run()


def schedule(stats):
    """the walk's schedule without what follows the device: for the run-to-run comparison of a seed"""
    return [(e["op"], e.get("seq") or e.get("seqs") or e.get("dst"), e.get("n"), e.get("refusal")) for e in stats["log"]]


def counts(stats):
    """what a live walk's statistics share with its dry walk's"""
    return dict(stats["ops"]), dict(stats["refusals"]), stats["calls"]


def coverage(stats):
    """what a walk's statistics lack of what every walk is to hold (dry or live); [] when nothing is missing"""
    ops, cross = stats["ops"], stats["cross"]
    bad = [f"{k}: {ops[k]} times" for k in OP_KINDS if ops[k] < 3]
    if ops["speculate_q8"] < 1:
        bad.append("no speculate_q8 loop")
    bad += [f"no refusal of the kind {k} at {c}" for k in REFUSALS for c in REFUSED_CALLS[k] if (k, c) not in stats["refused_calls"]]
    bad += [f"no {k} call across position 64" for k in ("verify_q8", "prefill_q8") if (k, 64) not in cross]
    if not any(e == 128 for _, e in cross):
        bad.append("no verify_q8 or prefill_q8 call across position 128")
    if stats["batch_sides"] < 1:
        bad.append("no transformer_batch_q8 call with rows on both sides of position 64")
    bad += [f"no transformer_batch_q8 call of {n} rows" for n in (1, BATCH_MAX) if n not in stats["batch_rows"]]
    bad += [f"no re-weight {d[0]} -> {d[1]} followed by prefill_q8" for d in ("ab", "ba") if d not in stats["reweight_prefill"]]
    if stats["longer"] < 1:
        bad.append("no prefill_q8 call longer than every earlier one on its runstate")
    bad += [f"no fork with n_pos {r} the source's depth" for r in ("below", "at", "above") if r not in stats["fork_rel"]]
    if stats["verify_temps"] != {False, True}:
        bad.append("verify_q8 not both at temperature 0 and with a temperature")
    return bad


def split_coverage(stats, split):
    """what a walk lacks of calls on both sides of the attention graph switch at position `split` (L2Z_ATTN_SPLIT_POS)"""
    done = [e for e in stats["log"] if "refusal" not in e and not e.get("skipped")]
    pos = [e["pos"] for e in done if e["op"] == "transformer"]
    bad = []
    if not any(p < split for p in pos) or not any(p >= split for p in pos):
        bad.append(f"transformer at {sorted(pos)}: not on both sides of {split}")
    for k in ("greedy_run", "sample_run"):   # (the positions each loop call really stepped, from the ids it returned)
        spans = [tuple(s) for e in done if e["op"] == k for s in e.get("spans", [])]
        if not any(a < split < b for a, b in spans):
            bad.append(f"no {k} call crosses {split}: {spans}")
    return bad
