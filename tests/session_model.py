"""A model of what the C ABI promises ACROSS calls, and a seeded random walk over every entry point that holds the library
to it.  No GPU in this module: tests/test_session_walk_cpu.py runs the walks "dry" (the device's outputs
replaced by the model's own expectation), tests/test_gpu_session_walk.py and scripts/fuzz_session.py run them on the device.

World: one synth_blob checkpoint per shape, N_SEQ contiguous runstates, N_SEQ paged ones from one KvPool that is too small
for all of them (so calls of the walk run it dry), one spare runstate for draws, the host sampler library.

Per sequence the model holds
    hist    the tokens it has consumed: KV rows below len(hist) are the sequence's, every row above is "whatever"
    lhist   the history its logits belong to (a fork copies the source's logits whatever n_pos is; None: never written)
    kind    contiguous or paged, and for a paged one the pages it holds (the model's own page names, shared after a fork)
    snap    the last bit-snapshot of its logits and caches
    m       one orc.Model, fed exactly the tokens the sequence consumed (replayed from the common prefix on fork / rewind)
The reference is the CPU oracle and nothing else.

The schedule -- which call, which runstates in which order, row counts, rewinds, temperatures, coins -- is drawn from
np.random.default_rng([seed, ...]) and never looks at device output; only the token ids the sequences consume (and with them
the accepted counts) follow what the device emitted.

After every call (live):
    value      every touched sequence's logits against its oracle at LOGIT_ATOL + LOGIT_RTOL * max|z| (test_gpu_parity.py);
               every readable verify_logits row at the same bar; l2z_score's log-probs at twice the bar (test_gpu_score.py)
    ids        where the oracle's top-2 margin exceeds the bar the id is the oracle's argmax; a sampled id whose logits
               can be read afterwards is l2z_sample_batch's on those logits with the same controls; accepted counts and
               paths are recomputed from out_next by the header's verdict rule
    footprint  bit for bit: a runstate absent from the call keeps its logits and every cache row, a present one every row
               outside the range its header names as written (a paged one is read through the logical view; rows of pages
               attached by the call are the page's, rows of pages given back read as 0)
    pages      n_free == n_pages - |union of attached pages|; every table attached exactly where the model expects, equal
               ids exactly where the model says a page is shared; a refused call leaves all of it as it was
At the end: rows below every sequence's depth against its oracle's KV rows at KV_TOL, everything closed, the pool whole.
"""
import ctypes as C
import os
import time
from collections import Counter

import numpy as np

from test_gpu_parity import LOGIT_ATOL, LOGIT_RTOL

KV_TOL = 2e-5        # tests/test_gpu_verify.py
PAGE = 64            # L2Z_KV_PAGE
N_SEQ = 12
BATCH_MAX, WIDE_MAX = 16, 128
OK, ERR_INVALID, ERR_OOM, ERR_STATE = 0, -1, -4, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED_W = 23

SHAPES = {
    # head size 48, 3 query heads per kv head; seq_len 160 = two pages and a last one of 32 rows
    "kvmul3": dict(dim=288, hidden_dim=768, n_layers=2, n_heads=6, n_kv_heads=2, vocab_size=1024, seq_len=160),
    # head size 64, 4 query heads per kv head; five pages
    "hs64": dict(dim=512, hidden_dim=1408, n_layers=2, n_heads=8, n_kv_heads=2, vocab_size=1024, seq_len=320),
}
# pages of the pool.  60 % of N_SEQ x pages-per-sequence (22 and 36) never ran dry in the dry runs -- forks, rewinds and
# re-created runstates keep most sequences in their first two pages, the peak use was 15 and 24 pages -- so the sizes were
# taken down until every walk of tests/test_session_walk_cpu.py meets L2Z_ERR_OOM while most paged calls still pass
POOL_PAGES = {"kvmul3": 14, "hs64": 16}

ROW_TOTALS = (16, 17, 32, 33, 64, 65)   # totals of the many-row calls land on both sides of these
WIDE_KINDS = ("prefill_batch", "transformer_wide", "transformer_wide_async", "wide_run", "verify_wide", "step_mixed")
REFUSALS = ("paged_nonwide", "mixed_kinds", "past_end", "bad_token", "duplicate", "shared_write", "short_pages")
# every kind of operation a walk must hold at least three times
OP_KINDS = ("transformer", "prefill", "score", "greedy_run", "sample_run", "verify", "verify_sample", "verify_tree",
            "transformer_batch", "verify_batch") + WIDE_KINDS + (
            "argmax", "argmax_batch", "sample_batch", "probs", "logits",
            "fork_cc", "fork_cp", "fork_pc", "fork_pp", "trim", "rewind", "recreate", "recreate_owner", "close_paged")
TEMPS = (0.0, 0.0, 0.4, 1.0)
TOP_PS = (0.0, 0.5, 0.9, 1.0)


class WalkFailure(AssertionError):
    """seed, index of the first failing operation, the failures and the log of operations (Python literals)"""

    def __init__(self, seed, index, failures, log):
        self.seed, self.index, self.failures, self.log = seed, index, failures, log
        lines = "\n".join(repr(e) for e in log[: index + 1][-12:])
        super().__init__(f"walk seed={seed!r} failed at operation {index} ({len(failures)} failures): {failures[:6]!r}\n"
                         f"replay: session_model.run(world, seed={seed!r}, stop_at={index}); the last operations:\n{lines}")


def host_sampler():
    """the host samplers of llama2.zig_amd/host (l2zh_sample_coin, l2zh_sample_top_p_coin)"""
    path = os.path.join(ROOT, "llama2.zig_amd", "host", "libllama2_host.so")
    if not os.path.exists(path):
        import __graft_entry__ as ge
        ge.build()
    L = C.CDLL(path)
    fp = C.POINTER(C.c_float)
    L.l2zh_sample_coin.restype = C.c_size_t
    L.l2zh_sample_coin.argtypes = [fp, C.c_size_t, C.c_float]
    L.l2zh_sample_top_p_coin.restype = C.c_size_t
    L.l2zh_sample_top_p_coin.argtypes = [fp, C.c_size_t, C.c_float, C.c_float, fp]
    return L


def host_token(H, probs, top_p, coin):
    probs = np.ascontiguousarray(probs, np.float32)
    pp = probs.ctypes.data_as(C.POINTER(C.c_float))
    if top_p in (0.0, 1.0):
        return int(H.l2zh_sample_coin(pp, probs.size, C.c_float(coin)))
    return int(H.l2zh_sample_top_p_coin(pp, probs.size, C.c_float(top_p), C.c_float(coin), None))


def first_max(z):
    """l2z_argmax's rule on finite rows: strict '>', the lowest index wins"""
    return int(np.flatnonzero(z == z.max())[0])


def accept(tokens, nxt):
    """l2z_verify's verdict: the number of leading guesses that equal the row before's out_next"""
    a = 0
    while a + 1 < len(tokens) and int(tokens[a + 1]) == int(nxt[a]):
        a += 1
    return a


def tree_verdict(tokens, parent, nxt):
    """l2z_verify_tree's verdict: cur = 0; while cur has a child c with tokens[c] == out_next[cur], cur = c"""
    path, cur = [0], 0
    while True:
        kids = [c for c in range(1, len(tokens)) if parent[c] == cur and int(tokens[c]) == int(nxt[cur])]
        if not kids:
            return path
        cur = kids[0]
        path.append(cur)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class World:
    """what the walks of one shape share: config, checkpoint, (live) weights; gpu=None: a dry world"""

    def __init__(self, ck, orc, shape, gpu=None, pool_pages=None):
        self.ck, self.orc, self.gpu, self.shape = ck, orc, gpu, shape
        self.cfg = ck.Config(**SHAPES[shape])
        self.blob = ck.synth_blob(self.cfg, False, SEED_W)
        self.pool_pages = POOL_PAGES[shape] if pool_pages is None else pool_pages
        self.H = host_sampler()
        self.w = gpu.Weights(self.cfg, self.blob, False) if gpu is not None else None
        self.memo = {}   # history -> the oracle's logits behind it (shared by the walks of the shape)

    def close(self):
        if self.w is not None:
            self.w.close()
            self.w = None


class Seq:
    def __init__(self, idx, paged, n_slots):
        self.idx, self.paged = idx, paged
        self.name = ("p" if paged else "c") + str(idx)
        self.rs = None
        self.m, self.mh = None, []
        self.pages = [None] * n_slots
        self.reset()

    def reset(self):
        self.hist, self.lhist, self.next_tok, self.g, self.snap = [], None, None, None, None
        self.fresh = set()


class Walk:
    def __init__(self, world, seed, n_ops=150, log=None, stop_at=None):
        self.W, self.seed, self.n_ops, self.say, self.stop_at = world, seed, n_ops, log, stop_at
        self.cfg, self.gpu, self.live = world.cfg, world.gpu, world.gpu is not None
        self.V, self.L = self.cfg.vocab_size, self.cfg.seq_len
        self.kvd = self.cfg.dim // self.cfg.n_heads * self.cfg.n_kv_heads
        self.n_slots = (self.L + PAGE - 1) // PAGE
        self.rng = np.random.default_rng([int(seed), 0x5E55])
        self.seqs = [Seq(i, False, self.n_slots) for i in range(N_SEQ)] + [Seq(i, True, self.n_slots) for i in range(N_SEQ)]
        self.refs, self.page_names = Counter(), 0
        self.pool = self.spare = None
        self.log, self.failures, self.first_bad = [], [], None
        self.st = dict(ops=Counter(), refusals=Counter(), id_total=0, id_under=0, worst=0.0, worst_at="", owner_moved=set(),
                       oom=0, calls=0)
        self.prev_owner = None
        self.owner = {}    # scratch family -> the sequence that owns it (states[0] of the family's last call)
        self.cur = None    # the log entry of the running operation

    # ---- plumbing ----------------------------------------------------------------------------------------------------
    @property
    def free(self):
        return self.W.pool_pages - len(self.refs)

    def fail(self, msg):
        self.failures.append((len(self.log) - 1, msg))
        if self.first_bad is None:
            self.first_bad = len(self.log) - 1
        if self.say:
            self.say(f"    FAIL {msg}")

    def make(self, q):
        if self.live:
            q.rs = self.gpu.RunState(self.cfg, pool=self.pool) if q.paged else self.gpu.RunState(self.cfg)
        if q.m is None:
            q.m = self.W.orc.Model(self.cfg.as_i32(), self.W.blob, False)
        q.reset()

    def feed(self, q, hist, memo=True):
        """q's oracle consumes hist (from the longest prefix it already holds); returns the last logits"""
        k, n = 0, min(len(q.mh), len(hist) - 1)   # (the last token always runs again: its logits are wanted)
        while k < n and q.mh[k] == hist[k]:
            k += 1
        z = None
        for p in range(k, len(hist)):
            z = q.m.transformer(int(hist[p]), p)
            if memo:
                self.W.memo[tuple(hist[: p + 1])] = z
        q.mh = list(hist)
        return z

    def olog(self, q, hist):
        """the oracle's logits behind `hist` (through q's own Model)"""
        hist = tuple(int(t) for t in hist)
        z = self.W.memo.get(hist)
        return z if z is not None else self.feed(q, hist)

    def ogreedy(self, q, hist, k):
        """the oracle's greedy continuation of hist, k tokens"""
        hist, out = list(hist), []
        for _ in range(k):
            out.append(first_max(self.olog(q, hist)))
            hist.append(out[-1])
        return out

    def bar(self, z):
        return LOGIT_ATOL + LOGIT_RTOL * float(np.abs(z).max())

    def value(self, what, got, ref, factor=1.0, bar=None):
        bar = factor * (self.bar(ref) if bar is None else bar)
        with np.errstate(invalid="ignore"):
            err = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())
        r = err / bar if np.isfinite(err) else np.inf
        kind = "worst_kv" if "cache" in what else "worst_logits"
        self.st[kind] = max(self.st.get(kind, 0.0), r)
        if r > self.st["worst"]:
            self.st["worst"], self.st["worst_at"] = r, f"op {len(self.log) - 1} {what}"
        self.cur["ratio"] = max(self.cur.get("ratio", 0.0), round(r, 4))
        if not r <= 1.0:
            self.fail(f"{what}: |got - oracle| = {err:.3e} > bar {bar:.3e}")

    def ident(self, what, got, z):
        """an id taken at temperature 0 from a row whose oracle logits are z"""
        top = np.partition(z, -2)[-2:]
        self.st["id_total"] += 1
        if float(top[1] - top[0]) > self.bar(z):
            if int(got) != first_max(z):
                self.fail(f"{what}: id {int(got)}, the oracle's argmax is {first_max(z)} at margin {float(top[1] - top[0]):.3e}")
        else:
            self.st["id_under"] += 1

    def draw(self, z, temp, top_p, coin):
        """the host sampler's token on the logits z (dry runs: the model's expectation of a device draw)"""
        if temp == 0:
            return first_max(z)
        x = (z / np.float32(temp)).astype(np.float32)
        p = np.exp(x - x.max()).astype(np.float32)
        return host_token(self.W.H, p / p.sum(dtype=np.float32), top_p, coin)

    def dev_draw(self, what, got, z_dev, temp, top_p, coin, z_orc):
        """live: the id `got` the device took from logits it lets us read back (z_dev)"""
        if temp == 0:
            self.ident(what, got, z_orc)
            want = first_max(z_dev)
        else:
            self.spare.write_logits(z_dev)
            want = int(self.gpu.sample_batch([self.spare], temp, top_p, coin)[0])
        if int(got) != want:
            self.fail(f"{what}: id {int(got)}, l2z_sample_batch draws {want} from the same logits (t {temp} p {top_p} coin {coin})")

    def wrong(self, t):
        return (int(t) - 2 + 1) % (self.V - 2) + 2

    # ---- the page model ---------------------------------------------------------------------------------------------
    def pg_slots(self, a, b):
        return range(a // PAGE, (b - 1) // PAGE + 1) if a < b else range(0)

    def pg_attach(self, seqs, ranges):
        """kv_attach's verdict for a wide call on paged sequences, and on OK its effect on the model"""
        if not seqs[0].paged:
            return OK
        need = 0
        for q, (a, b) in zip(seqs, ranges):
            if any(q.pages[p] is not None and self.refs[q.pages[p]] > 1 for p in self.pg_slots(a, b)):
                return ERR_STATE
            need += sum(q.pages[p] is None for p in self.pg_slots(a, b))
        if need > self.free:
            return ERR_OOM
        for q, (a, b) in zip(seqs, ranges):
            for p in self.pg_slots(a, b):
                if q.pages[p] is None:
                    self.page_names += 1
                    q.pages[p] = self.page_names
                    self.refs[self.page_names] = 1
                    q.fresh.add(p)
                    self.st["top_slot"] = max(self.st.get("top_slot", 0), p)
        return OK

    def pg_release(self, q, n_pos=0):
        """q lets go of every page wholly at or above n_pos; its snapshot reads 0 there from now on"""
        for p in range((n_pos + PAGE - 1) // PAGE, self.n_slots):
            if q.pages[p] is not None:
                self.refs[q.pages[p]] -= 1
                if self.refs[q.pages[p]] == 0:
                    del self.refs[q.pages[p]]
                q.pages[p] = None
                if q.snap is not None:
                    q.snap[1][:, p * PAGE:(p + 1) * PAGE, :] = 0
                    q.snap[2][:, p * PAGE:(p + 1) * PAGE, :] = 0

    # ---- device state ------------------------------------------------------------------------------------------------
    def read(self, q):
        n = self.cfg.n_layers * self.L * self.kvd
        shape = (self.cfg.n_layers, self.L, self.kvd)
        return [bits(q.rs.logits()), bits(q.rs.read("key_cache", 0, n)).reshape(shape).copy(),
                bits(q.rs.read("value_cache", 0, n)).reshape(shape).copy()]

    def settle(self, touched):
        """after a call: touched = {seq: (lo, hi) rows the header names as written, or None: any row} -- value, footprint, pages"""
        if not self.live:
            for q in self.seqs:
                q.fresh.clear()
            return
        for q in self.seqs:
            if q.rs is None:
                continue
            new = self.read(q)
            old = q.snap
            if old is not None and not (q in touched and touched[q] is None):
                keep = np.ones(self.L, bool)
                if q in touched:
                    keep[touched[q][0]: touched[q][1]] = False
                for p in q.fresh:
                    keep[p * PAGE:(p + 1) * PAGE] = False
                for name, a, b in (("key", old[1], new[1]), ("value", old[2], new[2])):
                    if not np.array_equal(a[:, keep, :], b[:, keep, :]):
                        rows = np.flatnonzero(keep)[np.any(a[:, keep, :] != b[:, keep, :], axis=(0, 2))]
                        self.fail(f"{q.name}: {name} cache rows {rows[:8].tolist()} changed outside the call's range "
                                  f"{touched.get(q, 'absent')}")
                if q not in touched and not np.array_equal(old[0], new[0]):
                    self.fail(f"{q.name}: logits changed by a call it took no part in")
            q.snap = new
            q.fresh.clear()
            if q in touched and q.lhist is not None:
                self.value(f"{q.name} logits", new[0].view(np.float32), self.olog(q, q.lhist))
        self.check_pages()

    def check_pages(self):
        ids = {}
        for q in self.seqs:
            if not q.paged or q.rs is None:
                continue
            tab = q.rs.pages().tolist()
            if [t >= 0 for t in tab] != [p is not None for p in q.pages]:
                self.fail(f"{q.name}: page table {tab}, the model expects pages at {[p is not None for p in q.pages]}")
                continue
            for t, p in zip(tab, q.pages):
                if p is not None and ids.setdefault(p, t) != t:
                    self.fail(f"{q.name}: page {t} where a shared page {ids[p]} is expected")
        if len(set(ids.values())) != len(ids):
            self.fail(f"two private pages of the model are one page of the pool: {ids}")
        n_free = self.pool.info()["n_free"]
        if n_free != self.W.pool_pages - len(set(ids.values())) or n_free != self.free:
            self.fail(f"n_free = {n_free}: {len(set(ids.values()))} pages attached of {self.W.pool_pages}, the model has {self.free} free")

    def refused(self, kind, code, fn, note=""):
        """a call the model expects to be refused with `code`: the code comes back and nothing changes"""
        self.st["refusals"][kind] += 1
        self.st["oom"] += code == ERR_OOM
        self.cur.update(refusal=kind, code=code, note=note)
        if self.live:
            try:
                fn()
                self.fail(f"{kind}: the call passed, expected code {code}")
            except self.gpu.L2ZError as e:
                if e.code != code:
                    self.fail(f"{kind}: code {e.code}, expected {code} ({e})")
        self.settle({})

    # ---- choosing ----------------------------------------------------------------------------------------------------
    def alive(self, paged):
        return [q for q in self.seqs if q.paged == paged]

    def pick(self, paged, n):
        pool = self.alive(paged)
        return [pool[i] for i in self.rng.permutation(len(pool))[:n]]

    def deepest(self, paged, qs):
        """every other time: instead of qs, as many of the deepest sequences of the kind that still have room for a long
        prompt -- so that some sequences reach their last pages"""
        if self.rng.random() < 0.5:
            return qs
        room = [q for q in self.alive(paged) if len(q.hist) + self.L * 2 // 5 <= self.L]
        room.sort(key=lambda q: (-len(q.hist), q.idx))
        return room[: len(qs)] or qs

    def plan(self, q, n, tokens=None):
        """where q's next n rows go -- on from its depth or, now and then, a rewind -- and the tokens it is fed there"""
        d = len(q.hist)
        pos0 = d
        if d + n > self.L or self.rng.random() < 0.12:
            pos0 = int(self.rng.integers(0, max(min(d, self.L - n), 0) + 1))
        toks = self.rng.integers(2, self.V, n).astype(np.int32) if tokens is None else np.asarray(tokens, np.int32)
        if pos0 == 0:
            toks[0] = 1
        elif pos0 == d and q.next_tok is not None and tuple(q.hist) == q.lhist and self.rng.random() < 0.7:
            toks[0] = q.next_tok
        if pos0 < d:
            self.cur["rewind"] = self.cur.get("rewind", 0) + 1
        return pos0, toks

    def split(self, total, n, cap=None):
        """total rows over n sequences, each at least 1 (and at most cap)"""
        parts = np.ones(n, np.int64)
        for _ in range(total - n):
            ok = np.flatnonzero(parts < (cap or total))
            if ok.size == 0:
                break
            parts[self.rng.choice(ok)] += 1
        return parts.tolist()

    def consume(self, q, pos0, toks):
        q.hist = q.hist[:pos0] + [int(t) for t in toks]
        q.lhist, q.g = tuple(q.hist), None

    def controls(self, n, rows=None):
        """temperature / top_p per sequence (None: the all-greedy NULL form) and coins per row"""
        if self.rng.random() < 0.4:
            return None, None, None
        t = [float(self.rng.choice(TEMPS)) for _ in range(n)]
        p = [float(self.rng.choice(TOP_PS)) for _ in range(n)]
        c = [self.rng.random(r, dtype=np.float32) for r in (rows or [1] * n)]
        return t, p, c

    # ---- single-sequence calls (contiguous) ------------------------------------------------------------------------
    def op_transformer(self):
        q, = self.pick(False, 1)
        pos0, t = self.plan(q, 1)
        self.cur.update(seq=q.name, pos=pos0, tok=int(t[0]))
        if self.live:
            q.rs.transformer(int(t[0]), pos0, self.W.w)
        self.consume(q, pos0, t)
        q.next_tok = None
        self.settle({q: (pos0, pos0 + 1)})

    def op_prefill(self, score=False):
        q, = self.pick(False, 1)
        n = int(self.rng.integers(1, 71))
        n = min(n, self.L)
        pos0, t = self.plan(q, n)
        self.cur.update(seq=q.name, pos=pos0, n=n)
        base = q.hist[:pos0]
        if score:
            tg = np.append(t[1:], -1).astype(np.int32)
            if self.rng.random() < 0.5:
                tg = self.rng.integers(0, self.V, n).astype(np.int32)
                tg[self.rng.random(n) < 0.2] = -1
            zs = [self.olog(q, base + t[: i + 1].tolist()) for i in range(n)]
            self.owner["score"] = q
            if self.live:
                lp, top = q.rs.score(t, pos0, self.W.w, targets=tg)
                for i, z in enumerate(zs):
                    z64 = z.astype(np.float64)
                    ref = 0.0 if tg[i] < 0 else z64[tg[i]] - (z64.max() + np.log(np.exp(z64 - z64.max()).sum()))
                    self.value(f"{q.name} score log-prob {i}", lp[i], ref, factor=2.0, bar=self.bar(z))
                    self.ident(f"{q.name} score top-1 {i}", top[i], z)
            else:
                for z in zs:
                    self.ident("", first_max(z), z)
        elif self.live:
            q.rs.prefill(t, pos0, self.W.w)
        self.consume(q, pos0, t)
        q.next_tok = None
        self.settle({q: (pos0, pos0 + n)})

    def op_score(self):
        self.op_prefill(score=True)

    def op_greedy_run(self, sampled=False):
        q, = self.pick(False, 1)
        going = [x for x in self.alive(False) if x.g is not None and not x.g["done"] and x.g["pos"] < self.L]
        if going and self.rng.random() < 0.7:   # a loop that is under way goes on, in mid-sequence
            q = going[int(self.rng.integers(0, len(going)))]
        g = q.g
        if g is None or g["done"] or g["pos"] >= self.L or self.rng.random() < 0.3:
            n_p = int(self.rng.choice([0, 0, 1, 3, 4, 6, 9]))
            g = dict(prompt=self.rng.integers(2, self.V, n_p).tolist(), pos=0, tok=1, done=False)
            if self.live:
                q.rs.greedy_begin(g["prompt"])
            self.cur["begin"] = g["prompt"]
        want = int(self.rng.integers(1, 13)) if self.rng.random() < 0.6 else int(self.rng.integers(13, 49))
        n = min(want, self.L - g["pos"])
        temp = float(self.rng.choice(TEMPS[1:])) if sampled else 0.0
        top_p = float(self.rng.choice(TOP_PS))
        coins = self.rng.random(want, dtype=np.float32)
        null_coins = temp == 0 and want % 2 == 0
        self.cur.update(seq=q.name, pos=g["pos"], n=want, temp=temp, top_p=top_p)
        if self.live:
            out = q.rs.sample_run(self.W.w, want, temp, top_p, None if null_coins else coins) \
                if sampled else q.rs.greedy_run(self.W.w, want)
            out = out.tolist()
        hist, tok, ids = q.hist[: g["pos"]], g["tok"], []
        for i in range(n):
            hist = hist + [tok]
            z = self.olog(q, hist)
            pos = g["pos"] + i
            if self.live:
                if i >= len(out):
                    self.fail(f"{q.name}: the loop produced {len(out)} ids, expected {n}")
                    break
                tok = out[i]
                if pos < len(g["prompt"]):
                    if tok != g["prompt"][pos]:
                        self.fail(f"{q.name}: step at prompt position {pos} gave {tok}, the prompt holds {g['prompt'][pos]}")
                elif temp == 0:
                    self.ident(f"{q.name} loop id {i}", tok, z)
            else:
                tok = g["prompt"][pos] if pos < len(g["prompt"]) else self.draw(z, temp, top_p, float(coins[i]))
                if pos >= len(g["prompt"]) and temp == 0:
                    self.ident("", tok, z)
            ids.append(tok)
            if tok == 1:
                g["done"] = True
                break
        if self.live and len(out) != len(ids):
            self.fail(f"{q.name}: the loop produced {len(out)} ids, expected {len(ids)}")
        lo = g["pos"]
        self.consume(q, 0, hist)
        g["pos"], g["tok"] = lo + len(ids), ids[-1]
        q.g, q.next_tok = g, ids[-1]
        self.settle({q: (lo, lo + n)})
        if self.live and sampled and temp > 0 and g["pos"] - 1 >= len(g["prompt"]):
            got = int(self.gpu.sample_batch([q.rs], temp, top_p, float(coins[len(ids) - 1]))[0])
            if got != ids[-1]:
                self.fail(f"{q.name}: the loop's last id {ids[-1]}, l2z_sample_batch draws {got} from its logits")

    def op_sample_run(self):
        self.op_greedy_run(sampled=True)

    def guesses(self, q, base, n, a_plan):
        """n - 1 guesses behind base: the oracle's greedy continuation, guess a_plan (0-based) made wrong"""
        g = self.ogreedy(q, base, n - 1)
        if a_plan < n - 1:
            g[a_plan] = self.wrong(g[a_plan])
        return g

    def op_verify(self, sampled=False):
        q, = self.pick(False, 1)
        n = int(self.rng.integers(1, BATCH_MAX + 1))
        pos0, t0 = self.plan(q, n)
        temp = float(self.rng.choice(TEMPS[1:])) if sampled else 0.0
        top_p = float(self.rng.choice(TOP_PS))
        coins = self.rng.random(n, dtype=np.float32)
        base = q.hist[:pos0] + [int(t0[0])]
        toks = [int(t0[0])] + self.guesses(q, base, n, int(self.rng.integers(0, n)))
        self.cur.update(seq=q.name, pos=pos0, n=n, temp=temp, top_p=top_p)
        zs = [self.olog(q, q.hist[:pos0] + toks[: i + 1]) for i in range(n)]
        self.owner["batch"] = q
        if self.live:
            if sampled:
                nxt, a = q.rs.verify_sample(toks, pos0, self.W.w, temp, top_p, coins if temp > 0 or n % 2 else None)
            else:
                nxt, a = q.rs.verify(toks, pos0, self.W.w)
            for i in range(n):
                zd = q.rs.verify_logits(i)
                self.value(f"{q.name} verify row {i}", zd, zs[i])
                self.dev_draw(f"{q.name} verify row {i}", nxt[i], zd, temp, top_p, float(coins[i]), zs[i])
            if a != accept(toks, nxt):
                self.fail(f"{q.name}: accepted {a}, the verdict rule gives {accept(toks, nxt)} on {nxt.tolist()}")
        else:
            nxt = [self.draw(zs[i], temp, top_p, float(coins[i])) for i in range(n)]
            for i in range(n):
                if temp == 0:
                    self.ident("", nxt[i], zs[i])
            a = accept(toks, nxt)
        self.cur["accepted"] = int(a)
        self.consume(q, pos0, toks[: a + 1])
        q.next_tok = int(nxt[a])
        self.settle({q: (pos0, pos0 + n)})

    def op_verify_sample(self):
        self.op_verify(sampled=True)

    def op_verify_tree(self):
        q, = self.pick(False, 1)
        n = int(self.rng.integers(2, BATCH_MAX + 1))
        pos0, t0 = self.plan(q, n)
        temp = float(self.rng.choice(TEMPS))
        top_p = float(self.rng.choice(TOP_PS))
        base = q.hist[:pos0] + [int(t0[0])]
        chain = int(self.rng.integers(1, n))            # guesses on the first chain
        a_plan = int(self.rng.integers(0, chain + 1))
        right = self.ogreedy(q, base, chain)
        toks, parent = [int(t0[0])] + self.guesses(q, base, chain + 1, a_plan), [-1] + list(range(chain))
        if a_plan < chain and len(toks) < n:             # the right token as a sibling of the wrong guess
            toks.append(right[a_plan])
            parent.append(a_plan)
        while len(toks) < n:
            par = int(self.rng.integers(0, len(toks)))
            taken = {toks[c] for c in range(1, len(toks)) if parent[c] == par}
            t = int(self.rng.integers(2, self.V))
            while t in taken:
                t = self.wrong(t)
            toks.append(t)
            parent.append(par)
        depth = [0] * n
        paths = [[0]] * n
        for i in range(1, n):
            depth[i], paths[i] = depth[parent[i]] + 1, paths[parent[i]] + [i]
        coins = self.rng.random(max(depth) + 1, dtype=np.float32)
        zs = [self.olog(q, q.hist[:pos0] + [toks[p] for p in paths[i]]) for i in range(n)]
        self.cur.update(seq=q.name, pos=pos0, n=n, temp=temp, top_p=top_p, parent=parent)
        self.owner["batch"] = q
        if self.live:
            nxt, path, a = q.rs.verify_tree(toks, parent, pos0, self.W.w, temp, top_p, coins if temp > 0 or n % 2 else None)
            for i in range(n):
                zd = q.rs.verify_logits(i)
                self.value(f"{q.name} tree node {i}", zd, zs[i])
                self.dev_draw(f"{q.name} tree node {i}", nxt[i], zd, temp, top_p, float(coins[depth[i]]), zs[i])
            want = tree_verdict(toks, parent, nxt)
            if path.tolist() != want or a != len(want) - 1:
                self.fail(f"{q.name}: path {path.tolist()} accepted {a}, the verdict rule walks {want}")
            path = want
        else:
            nxt = [self.draw(zs[i], temp, top_p, float(coins[depth[i]])) for i in range(n)]
            for i in range(n):
                if temp == 0:
                    self.ident("", nxt[i], zs[i])
            path = tree_verdict(toks, parent, nxt)
        self.cur["accepted"] = len(path) - 1
        self.consume(q, pos0, [toks[p] for p in path])
        q.next_tok = int(nxt[path[-1]])
        self.settle({q: (pos0, pos0 + n)})

    # ---- groups --------------------------------------------------------------------------------------------------------
    def op_transformer_batch(self):
        qs = self.pick(False, int(self.rng.integers(1, N_SEQ + 1)))
        plans = [self.plan(q, 1) for q in qs]
        pos, tok = [p for p, _ in plans], [int(t[0]) for _, t in plans]
        self.cur.update(seqs=[q.name for q in qs], pos=pos)
        self.owner["batch"] = qs[0]
        if self.live:
            self.gpu.transformer_batch([q.rs for q in qs], tok, pos, self.W.w)
        for q, p, t in zip(qs, pos, tok):
            self.consume(q, p, [t])
            q.next_tok = None
        self.settle({q: (p, p + 1) for q, p in zip(qs, pos)})

    def wide_front(self, kind, qs, ranges, fn):
        """what every call of the wide family starts with: the pages (a refusal ends the operation: returns False) and
        whose scratch it runs on"""
        code = self.pg_attach(qs, ranges)
        if code != OK:
            self.refused("shared_write" if code == ERR_STATE else "short_pages", code, fn, note="natural")
            self.cur["rewind"] = 0
            return False
        if kind in WIDE_KINDS:
            if self.prev_owner is not None and self.prev_owner is not qs[0]:
                self.st["owner_moved"].add(kind)
            self.prev_owner = qs[0]
            self.owner["ragged" if kind == "prefill_batch" else "wide"] = qs[0]
        return True

    def rows_total(self, n, cap_each=None, cap=WIDE_MAX):
        """a total row count for n sequences: often right at one of ROW_TOTALS"""
        hi = min(cap, n * (cap_each or cap))
        total = int(self.rng.choice(ROW_TOTALS)) if self.rng.random() < 0.6 else int(self.rng.integers(n, hi + 1))
        return self.split(max(min(total, hi), n), n, cap_each)

    def op_prefill_batch(self):
        paged = bool(self.rng.integers(0, 2))
        qs = self.pick(paged, int(self.rng.integers(1, N_SEQ + 1)))
        if self.rng.random() < 0.4:   # two long prompts (a quarter to two fifths of seq_len): sequences that reach their upper pages
            qs = self.deepest(paged, qs[:2])
            ns = [int(self.rng.integers(self.L // 4, self.L * 2 // 5 + 1)) for _ in qs]
        else:
            ns = [min(m, 70, self.L) for m in self.rows_total(len(qs))]
        plans = [self.plan(q, m) for q, m in zip(qs, ns)]
        pos0, toks = [p for p, _ in plans], [t for _, t in plans]
        self.cur.update(seqs=[q.name for q in qs], pos=pos0, n=ns, rows=sum(ns))
        fn = lambda: self.gpu.prefill_batch([q.rs for q in qs], toks, pos0, self.W.w)
        if not self.wide_front("prefill_batch", qs, [(p, p + m) for p, m in zip(pos0, ns)], fn):
            return
        if self.live:
            fn()
        for q, p, t in zip(qs, pos0, toks):
            self.consume(q, p, t)
            q.next_tok = None
        self.settle({q: (p, p + m) for q, p, m in zip(qs, pos0, ns)})

    def op_transformer_wide(self, want_next=True):
        paged = bool(self.rng.integers(0, 2))
        qs = self.pick(paged, int(self.rng.integers(1, N_SEQ + 1)))
        plans = [self.plan(q, 1) for q in qs]
        pos, tok = [p for p, _ in plans], [int(t[0]) for _, t in plans]
        kind = "transformer_wide" if want_next else "transformer_wide_async"
        self.cur.update(seqs=[q.name for q in qs], pos=pos)
        fn = lambda: self.gpu.transformer_wide([q.rs for q in qs], tok, pos, self.W.w, want_next=want_next)
        if not self.wide_front(kind, qs, [(p, p + 1) for p in pos], fn):
            return
        nxt = fn() if self.live else None
        for j, (q, p, t) in enumerate(zip(qs, pos, tok)):
            self.consume(q, p, [t])
            q.next_tok = None
            if want_next:
                z = self.olog(q, q.hist)
                q.next_tok = int(nxt[j]) if self.live else first_max(z)
                self.ident(f"{q.name} out_next", q.next_tok, z)
        self.settle({q: (p, p + 1) for q, p in zip(qs, pos)})
        if self.live and want_next:
            for j, q in enumerate(qs):
                if int(nxt[j]) != first_max(q.snap[0].view(np.float32)):
                    self.fail(f"{q.name}: out_next {int(nxt[j])} is not the argmax of the logits the call left")

    def op_transformer_wide_async(self):
        self.op_transformer_wide(want_next=False)

    def op_wide_run(self):
        paged = bool(self.rng.integers(0, 2))
        qs = self.pick(paged, int(self.rng.integers(1, N_SEQ + 1)))
        n, steps = len(qs), int(self.rng.integers(1, 7))
        plans = [self.plan(q, steps) for q in qs]
        pos0, first = [p for p, _ in plans], [int(t[0]) for _, t in plans]
        temp, top_p, _ = self.controls(n)
        if temp is not None and all(t == 0 for t in temp):
            temp[0] = 1.0   # greedy and sampled rows mixed
        coins = self.rng.random((steps, n), dtype=np.float32)
        self.cur.update(seqs=[q.name for q in qs], pos=pos0, steps=steps, temp=temp, top_p=top_p)
        fn = lambda: self.gpu.wide_run([q.rs for q in qs], first, pos0, self.W.w, steps, temperature=temp, top_p=top_p,
                                       coins=None if temp is None else coins)
        if not self.wide_front("wide_run", qs, [(p, p + steps) for p in pos0], fn):
            return
        ids = fn() if self.live else np.zeros((steps, n), np.int32)
        for j, q in enumerate(qs):
            tj, pj = (0.0, 1.0) if temp is None else (temp[j], top_p[j])
            hist, tok = q.hist[: pos0[j]], first[j]
            for k in range(steps):
                hist = hist + [tok]
                z = self.olog(q, hist)
                if not self.live:
                    ids[k, j] = self.draw(z, tj, pj, float(coins[k, j]))
                if tj == 0:
                    self.ident(f"{q.name} wide_run step {k}", ids[k, j], z)
                tok = int(ids[k, j])
            self.consume(q, 0, hist)
            q.next_tok = tok
        self.settle({q: (p, p + steps) for q, p in zip(qs, pos0)})
        if self.live:
            for j, q in enumerate(qs):   # the last step's draw, from the logits the run left
                tj, pj = (0.0, 1.0) if temp is None else (temp[j], top_p[j])
                got = int(self.gpu.sample_batch([q.rs], tj, pj, float(coins[-1, j]))[0])
                if got != int(ids[-1, j]):
                    self.fail(f"{q.name}: wide_run's last id {int(ids[-1, j])}, l2z_sample_batch draws {got} from its logits")

    def verify_rows(self, kind, paged):
        cap = BATCH_MAX if kind == "verify_batch" else WIDE_MAX
        n = int(self.rng.integers(1, N_SEQ + 1))
        qs = self.pick(paged, n)
        ns = self.rows_total(n, cap_each=BATCH_MAX, cap=cap) if cap > BATCH_MAX else self.split(int(self.rng.integers(n, cap + 1)), n)
        temp, top_p, coins = self.controls(n, ns)
        plans = [self.plan(q, m) for q, m in zip(qs, ns)]
        pos0 = [p for p, _ in plans]
        lists = []
        for q, m, (p, t0) in zip(qs, ns, plans):
            base = q.hist[:p] + [int(t0[0])]
            lists.append([int(t0[0])] + self.guesses(q, base, m, int(self.rng.integers(0, m))))
        self.cur.update(seqs=[q.name for q in qs], pos=pos0, n=ns, rows=sum(ns), temp=temp, top_p=top_p)
        call = (self.gpu.verify_batch if kind == "verify_batch" else self.gpu.verify_wide) if self.live else None
        fn = lambda: call([q.rs for q in qs], lists, pos0, self.W.w, temperature=temp, top_p=top_p, coin_lists=coins)
        if not self.wide_front(kind, qs, [(p, p + m) for p, m in zip(pos0, ns)], fn):
            return
        if kind == "verify_batch":
            self.owner["batch"] = qs[0]
        if self.live:
            nxts, acc = fn()
        r, new = 0, []
        for j, (q, m, p, toks) in enumerate(zip(qs, ns, pos0, lists)):
            tj, pj = (0.0, 1.0) if temp is None else (temp[j], top_p[j])
            zs = [self.olog(q, q.hist[:p] + toks[: i + 1]) for i in range(m)]
            if self.live:
                nxt = nxts[j]
                for i in range(m):
                    zd = qs[0].rs.verify_logits(r + i)
                    self.value(f"{q.name} {kind} row {r + i}", zd, zs[i])
                    self.dev_draw(f"{q.name} {kind} row {r + i}", nxt[i], zd, tj, pj, float(coins[j][i]) if coins else 0.0, zs[i])
                a = accept(toks, nxt)
                if int(acc[j]) != a:
                    self.fail(f"{q.name}: accepted {int(acc[j])}, the verdict rule gives {a} on {nxt.tolist()}")
            else:
                nxt = [self.draw(zs[i], tj, pj, float(coins[j][i]) if coins else 0.0) for i in range(m)]
                for i in range(m):
                    if tj == 0:
                        self.ident("", nxt[i], zs[i])
                a = accept(toks, nxt)
            new.append((q, p, toks[: a + 1], int(nxt[a])))
            r += m
        if self.live:
            for q in qs[1:]:   # the matrix is states[0]'s: the others have no row
                try:
                    q.rs.verify_logits(0)
                    self.fail(f"{q.name}: verify_logits_read answers on a runstate that is not states[0] of the {kind} call")
                except self.gpu.L2ZError as e:
                    if e.code != ERR_STATE:
                        self.fail(f"{q.name}: verify_logits_read code {e.code}, expected {ERR_STATE}")
        self.cur["accepted"] = [len(t) - 1 for _, _, t, _ in new]
        for q, p, t, nx in new:
            self.consume(q, p, t)
            q.next_tok = nx
        self.settle({q: (p, p + m) for q, p, m in zip(qs, pos0, ns)})

    def op_verify_batch(self):
        self.verify_rows("verify_batch", False)

    def op_verify_wide(self):
        self.verify_rows("verify_wide", bool(self.rng.integers(0, 2)))

    def op_step_mixed(self):
        paged = bool(self.rng.integers(0, 2))
        n = int(self.rng.integers(1, N_SEQ + 1)) if self.rng.random() < 0.6 else int(self.rng.integers(1, 4))
        qs = self.pick(paged, n)
        ns = [min(m, self.L) for m in self.rows_total(n)]
        for j in range(n):   # decode rows among the prompt chunks
            if self.rng.random() < 0.4:
                ns[j] = 1
        if self.rng.random() < 0.3:   # ... and long chunks, as prefill_batch's long prompts
            qs = self.deepest(paged, qs[:2]) + qs[2:]
            qs = qs[:2] + [q for q in qs[2:] if q not in qs[:2]]
            n = len(qs)
            ns = ns[:n]
            for j in range(min(n, 2)):
                ns[j] = int(self.rng.integers(self.L // 4, self.L * 2 // 5 + 1))
        temp, top_p, coins = self.controls(n)
        coins = None if coins is None else [float(c[0]) for c in coins]
        plans = [self.plan(q, m) for q, m in zip(qs, ns)]
        pos0, toks = [p for p, _ in plans], [t for _, t in plans]
        self.cur.update(seqs=[q.name for q in qs], pos=pos0, n=ns, rows=sum(ns), temp=temp, top_p=top_p)
        fn = lambda: self.gpu.step_mixed([q.rs for q in qs], toks, pos0, self.W.w, temperature=temp, top_p=top_p, coins=coins)
        if not self.wide_front("step_mixed", qs, [(p, p + m) for p, m in zip(pos0, ns)], fn):
            return
        nxt = fn() if self.live else None
        for j, (q, p, t) in enumerate(zip(qs, pos0, toks)):
            self.consume(q, p, t)
            tj, pj, cj = (0.0, 1.0, 0.0) if temp is None else (temp[j], top_p[j], coins[j])
            z = self.olog(q, q.hist)
            q.next_tok = int(nxt[j]) if self.live else self.draw(z, tj, pj, cj)
            if tj == 0:
                self.ident(f"{q.name} step_mixed id", q.next_tok, z)
        self.settle({q: (p, p + m) for q, p, m in zip(qs, pos0, ns)})
        if self.live:
            for j, q in enumerate(qs):
                tj, pj, cj = (0.0, 1.0, 0.0) if temp is None else (temp[j], top_p[j], coins[j])
                got = int(self.gpu.sample_batch([q.rs], tj, pj, cj)[0])
                if got != int(nxt[j]):
                    self.fail(f"{q.name}: step_mixed drew {int(nxt[j])}, l2z_sample_batch draws {got} from its logits")

    # ---- logits-only calls, on any subset, right after any call -----------------------------------------------------
    def readable(self):
        return [q for q in self.seqs if q.lhist is not None]

    def op_logits_only(self, kind):
        have = self.readable()
        if not have:
            return False
        if kind in ("argmax", "probs", "logits"):
            q = have[int(self.rng.integers(0, len(have)))]
            z = self.olog(q, q.lhist)
            self.cur.update(seq=q.name)
            if kind == "argmax":
                self.ident(f"{q.name} argmax", q.rs.argmax() if self.live else first_max(z), z)
                if self.live and q.rs.argmax() != first_max(q.rs.logits()):
                    self.fail(f"{q.name}: l2z_argmax {q.rs.argmax()} is not the argmax of l2z_logits_read's row")
            elif kind == "logits":
                if self.live:
                    self.value(f"{q.name} logits_read", q.rs.logits(), z)
            else:
                temp = float(self.rng.choice(TEMPS[2:]))
                self.cur.update(temp=temp)
                if self.live:
                    x = z.astype(np.float64) / temp
                    p = np.exp(x - x.max())
                    got = q.rs.probs(temp)
                    # a logit error e moves a probability by at most p (e^(2 e / t) - 1): the logits' bar through the softmax
                    self.value(f"{q.name} probs", got, p / p.sum(), bar=float(np.expm1(2 * self.bar(z) / temp)) * float((p / p.sum()).max()) + 1e-7)
        else:
            paged = bool(self.rng.integers(0, 2))
            same = [q for q in have if q.paged == paged] if self.rng.random() < 0.5 else have
            same = same or have
            qs = [same[i] for i in self.rng.permutation(len(same))[: int(self.rng.integers(1, min(len(same), BATCH_MAX) + 1))]]
            self.cur.update(seqs=[q.name for q in qs])
            zs = [self.olog(q, q.lhist) for q in qs]
            if kind == "argmax_batch":
                got = self.gpu.argmax_batch([q.rs for q in qs]) if self.live else [first_max(z) for z in zs]
                for q, t, z in zip(qs, got, zs):
                    self.ident(f"{q.name} argmax_batch", t, z)
            else:
                temp = [float(self.rng.choice(TEMPS)) for _ in qs]
                top_p = [float(self.rng.choice(TOP_PS)) for _ in qs]
                coins = self.rng.random(len(qs), dtype=np.float32)
                self.cur.update(temp=temp, top_p=top_p)
                if self.live:
                    got = self.gpu.sample_batch([q.rs for q in qs], temp, top_p, coins)
                    for q, t, tj, pj, cj, z in zip(qs, got, temp, top_p, coins, zs):
                        if tj == 0:
                            self.ident(f"{q.name} sample_batch", t, z)
                            want = first_max(q.rs.logits())
                        else:   # the header's own statement: the host sampler's walk on l2z_probs_read's probabilities
                            want = host_token(self.W.H, q.rs.probs(tj), pj, float(cj))
                        if int(t) != want:
                            self.fail(f"{q.name}: sample_batch {int(t)}, the host sampler draws {want} (t {tj} p {pj} coin {cj})")
                else:
                    for tj, z in zip(temp, zs):
                        if tj == 0:
                            self.ident("", first_max(z), z)
        self.settle({})
        return True

    # ---- state operations --------------------------------------------------------------------------------------------
    def op_fork(self, kind):
        dp, sp = kind[-2] == "p", kind[-1] == "p"     # fork_<dst><src>
        src = [q for q in self.alive(sp) if q.lhist is not None]
        if not src:
            return False
        s = src[int(self.rng.integers(0, len(src)))]
        if self.rng.random() < 0.6:   # the deepest: forks that share whole pages
            s = max(src, key=lambda q: len(q.hist))
        dsts = [q for q in self.alive(dp) if q is not s]
        d = dsts[int(self.rng.integers(0, len(dsts)))]
        depth = len(s.hist)
        edges = [e for e in (depth, PAGE - 1, PAGE, PAGE + 1, 2 * PAGE - 1, 2 * PAGE, 2 * PAGE + 1, depth // 2) if e <= depth]
        n_pos = int(self.rng.choice(edges)) if self.rng.random() < 0.7 else int(self.rng.integers(0, depth + 1))
        self.cur.update(dst=d.name, src=s.name, n_pos=n_pos)
        fn = lambda: self.gpu.runstate_fork(d.rs, s.rs, n_pos)
        if dp:
            whole = n_pos // PAGE if sp else 0
            back = sum(p is not None and self.refs[p] == 1 for p in d.pages)
            if (n_pos + PAGE - 1) // PAGE - whole > self.free + back:
                self.refused("short_pages", ERR_OOM, fn, note="natural, fork")
                return True
            self.pg_release(d, 0)
            for p in range(whole):
                d.pages[p] = s.pages[p]
                self.refs[s.pages[p]] += 1
            code = self.pg_attach([d], [(whole * PAGE, n_pos)])
            assert code == OK
        if self.live:
            fn()
        d.hist, d.lhist, d.next_tok, d.g = s.hist[:n_pos], s.lhist, None, None
        # (dst's rows >= n_pos are not touched; a paged dst reads 0 where it gave pages back, and its new private page is the page's)
        self.settle({d: (0, n_pos)})
        if self.live:
            if not np.array_equal(d.snap[0], s.snap[0]):
                self.fail(f"{d.name}: its logits are not {s.name}'s after the fork")
            for a, b in ((d.snap[1], s.snap[1]), (d.snap[2], s.snap[2])):
                if not np.array_equal(a[:, :n_pos, :], b[:, :n_pos, :]):
                    self.fail(f"{d.name}: cache rows below {n_pos} are not {s.name}'s after the fork")
        return True

    def op_trim(self):
        have = [q for q in self.alive(True) if any(p is not None for p in q.pages)]
        if not have:
            return False
        q = have[int(self.rng.integers(0, len(have)))]
        top = max(p for p in range(self.n_slots) if q.pages[p] is not None) * PAGE
        n_pos = int(self.rng.choice([0, top, top + 1, len(q.hist), int(self.rng.integers(0, self.L + 1))]))
        self.cur.update(seq=q.name, n_pos=n_pos)
        if self.live:
            q.rs.trim(n_pos)
        self.pg_release(q, n_pos)
        q.hist = q.hist[: min(len(q.hist), (n_pos + PAGE - 1) // PAGE * PAGE)]
        q.g = None
        self.settle({})
        return True

    def op_recreate(self, kind):
        """close a runstate and make it anew: any contiguous one, the owner of a scratch, or a paged one (its pages recycle)"""
        if kind == "recreate_owner":
            own = sorted({q.idx + N_SEQ * q.paged for q in self.owner.values()})
            if not own:
                return False
            q = self.seqs[own[int(self.rng.integers(0, len(own)))]]
        else:
            q, = self.pick(kind == "close_paged", 1)
        self.cur.update(seq=q.name, owns=[k for k, v in self.owner.items() if v is q])
        if self.live:
            q.rs.close()
        if q.paged:
            self.pg_release(q, 0)
        self.owner = {k: v for k, v in self.owner.items() if v is not q}
        if self.prev_owner is q:
            self.prev_owner = None
        self.make(q)
        self.settle({q: None})
        return True

    # ---- refusals ------------------------------------------------------------------------------------------------------
    def op_refusal(self):
        kind = REFUSALS[int(self.rng.integers(0, len(REFUSALS)))]
        g, w = self.gpu, self.W.w
        c, p = self.pick(False, 3), self.pick(True, 3)
        rs = lambda qs: [q.rs for q in qs]
        one = np.array([5], np.int32)
        if kind == "shared_write":
            have = [(q, s) for q in self.alive(True) for s in range(self.n_slots)
                    if q.pages[s] is not None and self.refs[q.pages[s]] > 1 and s * PAGE < len(q.hist)]
            if not have:
                kind = "duplicate"
            else:
                q, s = have[int(self.rng.integers(0, len(have)))]
                pos = int(self.rng.integers(s * PAGE, min((s + 1) * PAGE, len(q.hist))))
                which = int(self.rng.integers(0, 3))
                fn = [lambda: g.transformer_wide([q.rs], [5], [pos], w), lambda: g.step_mixed([q.rs], [[5, 6]], [pos], w),
                      lambda: g.verify_wide([q.rs], [[5, 6, 7]], [max(pos - 1, 0)], w)][which]
                return self.refused(kind, ERR_STATE, fn, note=f"{q.name} pos {pos} call {which}")
        if kind == "short_pages":
            have = [q for q in self.alive(True) if len(q.hist) < self.L and
                    sum(x is None for x in q.pages[len(q.hist) // PAGE:]) > self.free and
                    not any(x is not None and self.refs[x] > 1 for x in q.pages[len(q.hist) // PAGE:])]
            if not have:
                kind = "mixed_kinds"
            else:
                q = have[int(self.rng.integers(0, len(have)))]
                d = len(q.hist)
                t = self.rng.integers(2, self.V, self.L - d).astype(np.int32)
                which = int(self.rng.integers(0, 2))
                fn = [lambda: g.prefill_batch([q.rs], [t], [d], w), lambda: g.step_mixed([q.rs], [t], [d], w)][which]
                return self.refused(kind, ERR_OOM, fn, note=f"{q.name} rows {d} .. {self.L - 1} call {which}")
        which = int(self.rng.integers(0, 6))
        note = f"call {which}"
        if kind == "paged_nonwide":
            q = p[0]
            t = np.array([1, 5, 7], np.int32)
            fn = [lambda: q.rs.transformer(1, 0, w), lambda: q.rs.prefill(t, 0, w), lambda: q.rs.score(t, 0, w),
                  lambda: g.transformer_batch([q.rs], [1], [0], w), lambda: q.rs.verify(t, 0, w),
                  lambda: q.rs.greedy_run(w, 2)][which]
            code = ERR_INVALID
        elif kind == "mixed_kinds":
            qs = [c[0], p[0], c[1]] if which % 2 else [p[0], c[0]]
            n = len(qs)
            fn = [lambda: g.transformer_wide(rs(qs), [1] * n, [0] * n, w), lambda: g.prefill_batch(rs(qs), [one] * n, 0, w),
                  lambda: g.wide_run(rs(qs), [1] * n, [0] * n, w, 2), lambda: g.verify_wide(rs(qs), [one] * n, [0] * n, w),
                  lambda: g.step_mixed(rs(qs), [one] * n, [0] * n, w), lambda: g.transformer_wide(rs(qs), [1] * n, [0] * n, w, want_next=False)][which]
            code = ERR_INVALID
        elif kind == "past_end":
            q, L = c[0], self.L
            t = np.arange(2, 7, dtype=np.int32)
            fn = [lambda: q.rs.prefill(t, L - 4, w), lambda: q.rs.verify(t, L - 4, w), lambda: q.rs.transformer(5, L, w),
                  lambda: g.prefill_batch(rs(c), [t, t, t], [0, L - 4, 0], w), lambda: g.wide_run(rs(c), [5, 5, 5], [0, 0, L - 2], w, 3),
                  lambda: g.step_mixed(rs(c), [t, one, one], [L - 4, 0, 0], w)][which]
            code = ERR_STATE
        elif kind == "bad_token":
            q, bad = c[0], [self.V, -1][which % 2]
            t = np.array([1, 5, bad], np.int32)
            fn = [lambda: q.rs.prefill(t, 0, w), lambda: q.rs.verify(t, 0, w), lambda: q.rs.transformer(bad, 0, w),
                  lambda: g.transformer_batch(rs(c), [1, bad, 1], [0, 0, 0], w), lambda: g.transformer_wide(rs(c), [1, 1, bad], [0, 0, 0], w),
                  lambda: g.step_mixed(rs(c), [one, t, one], [0, 0, 0], w)][which]
            code = ERR_STATE
        else:
            kind = "duplicate"
            qs = [c[0], c[1], c[0]] if which % 2 else [p[0], p[0]]
            n = len(qs)
            fn = [lambda: g.transformer_wide(rs(qs), [1] * n, [0] * n, w), lambda: g.transformer_batch(rs([c[0], c[1], c[0]]), [1] * 3, [0] * 3, w),
                  lambda: g.prefill_batch(rs(qs), [one] * n, 0, w), lambda: g.verify_batch(rs([c[0], c[1], c[0]]), [one] * 3, [0] * 3, w),
                  lambda: g.step_mixed(rs(qs), [one] * n, [0] * n, w), lambda: g.verify_wide(rs(qs), [one] * n, [0] * n, w)][which]
            code = ERR_INVALID
        return self.refused(kind, code, fn, note=note)

    # ---- the walk ------------------------------------------------------------------------------------------------------
    MAIN = (("transformer", 4), ("prefill", 5), ("score", 4), ("greedy_run", 5), ("sample_run", 5), ("verify", 5),
            ("verify_sample", 5), ("verify_tree", 5), ("transformer_batch", 5), ("verify_batch", 5), ("prefill_batch", 9),
            ("transformer_wide", 6), ("transformer_wide_async", 6), ("wide_run", 7), ("verify_wide", 8), ("step_mixed", 9),
            ("fork_cc", 4), ("fork_cp", 4), ("fork_pc", 4), ("fork_pp", 6), ("trim", 5), ("recreate", 4), ("recreate_owner", 5),
            ("close_paged", 4), ("refusal", 17))
    AFTER = ("argmax", "argmax_batch", "sample_batch", "probs", "logits")

    def schedule_kinds(self):
        """the walk's main operations: a warm-up of calls that write rows, then every kind three times, one refusal in ten
        operations and the rest by the weights of MAIN, shuffled"""
        n_main = max(int(round(self.n_ops / 1.4)), 1)
        names = [k for k, _ in self.MAIN if k != "refusal"]
        weights = np.array([v for k, v in self.MAIN if k != "refusal"], np.float64)
        warm = ["prefill_batch", "step_mixed", "prefill", "prefill_batch", "greedy_run", "step_mixed", "verify_wide", "prefill_batch"]
        # (a fourth of the kinds that a dry pool or a shared page may refuse)
        body = names * 3 + list(WIDE_KINDS) + ["fork_cp", "fork_pp", "fork_pc"] + ["refusal"] * max(self.n_ops // 10, 1)
        fill = n_main - len(warm) - len(body)
        if fill > 0:
            body += [names[i] for i in self.rng.choice(len(names), fill, p=weights / weights.sum())]
        body = [body[i] for i in self.rng.permutation(len(body))]
        return (warm + body)[:n_main] if fill >= 0 else [body[i] for i in range(n_main)]

    def one(self, kind):
        self.cur = dict(i=len(self.log), op=kind)
        self.log.append(self.cur)
        self.st["calls"] += 1
        if kind in self.AFTER:
            done = self.op_logits_only(kind)
        elif kind.startswith("fork_"):
            done = self.op_fork(kind)
        elif kind in ("recreate", "recreate_owner", "close_paged"):
            done = self.op_recreate(kind)
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
            if self.live:
                self.pool = self.gpu.KvPool(self.cfg, self.W.pool_pages)
                self.spare = self.gpu.RunState(self.cfg)
            for q in self.seqs:
                self.make(q)
            self.settle({q: None for q in self.seqs})
            after = []
            follow = set(self.rng.choice(len(plan), min(max(self.n_ops - len(plan), 0), len(plan)), replace=False).tolist())
            for k, kind in enumerate(plan):
                if self.stop_at is not None and len(self.log) > self.stop_at:
                    break
                self.one(kind)
                self.st["min_free"] = min(self.st.get("min_free", self.free), self.free)
                if k in follow:
                    if not after:   # (every kind of them comes round before one comes twice)
                        after = [self.AFTER[i] for i in self.rng.permutation(len(self.AFTER))]
                    self.one(after.pop())
            self.finish()
        except WalkFailure:
            raise
        except Exception as e:   # a call the model expected to pass did not (or the walk itself broke): the state is unknown
            self.fail(f"{type(e).__name__}: {e}")
            self.close()
            raise WalkFailure(self.seed, self.first_bad, self.failures, self.log) from e
        self.st["wall"] = time.perf_counter() - t0
        self.st["seq_len"] = self.L
        self.st["log"] = self.log
        self.st["under_share"] = self.st["id_under"] / max(self.st["id_total"], 1)
        if self.failures:
            raise WalkFailure(self.seed, self.first_bad, self.failures, self.log)
        return self.st

    def finish(self):
        """every sequence's rows below its depth against its oracle's; then everything closes and the pool is whole"""
        self.cur = dict(i=len(self.log), op="end")
        self.log.append(self.cur)
        n = self.cfg.n_layers * self.L * self.kvd
        if self.live and self.stop_at is None:
            for q in self.seqs:
                d = len(q.hist)
                if d == 0:
                    continue
                if q.mh[:d] != q.hist:
                    self.feed(q, q.hist, memo=False)
                for name, got in (("key_cache", q.snap[1]), ("value_cache", q.snap[2])):
                    ref = q.m.state(name, n).reshape(self.cfg.n_layers, self.L, self.kvd)[:, :d, :]
                    self.value(f"{q.name} {name} rows below {d}", got.view(np.float32)[:, :d, :], ref, bar=KV_TOL)
        self.close()

    def close(self):
        for q in self.seqs:
            if q.rs is not None:
                q.rs.close()
                q.rs = None
            if q.m is not None:
                q.m.close()
                q.m = None
        if self.spare is not None:
            self.spare.close()
            self.spare = None
        if self.pool is not None:
            info = self.pool.info()
            if info["n_free"] != info["n_pages"]:
                self.fail(f"the pool reports {info['n_free']} of {info['n_pages']} pages free after every runstate closed")
            try:
                self.pool.close()
            except Exception as e:
                self.fail(f"pool.close(): {e}")
            self.pool = None


def run(world, seed, n_ops=150, log=None, stop_at=None):
    """One walk of n_ops operations; returns its statistics, raises WalkFailure.  stop_at=k: replay up to operation k"""
    return Walk(world, seed, n_ops=n_ops, log=log, stop_at=stop_at).run()


def schedule(stats):
    """the walk's schedule without what follows the device: for the run-to-run comparison of a seed"""
    return [(e["op"], e.get("seq") or e.get("seqs") or e.get("dst"), e.get("pos"), e.get("n"), e.get("refusal")) for e in stats["log"]]


def coverage(stats):
    """what a walk's statistics lack of what every walk is to hold (dry or live): every kind of operation three times, the
    scratch owner moved before every wide kind, a dry pool, few ids under the margin; [] when nothing is missing"""
    bad = [f"{k}: {stats['ops'][k]} times" for k in OP_KINDS if stats["ops"][k] < 3]
    bad += [f"{k}: never with another states[0] than the wide call before" for k in WIDE_KINDS if k not in stats["owner_moved"]]
    if stats["oom"] < 1 or stats["min_free"] != 0:
        bad.append(f"the pool never ran dry: {stats['oom']} L2Z_ERR_OOM, {stats['min_free']} pages free at the least")
    if stats["id_under"] > 0.05 * stats["id_total"]:
        bad.append(f"{stats['id_under']} of {stats['id_total']} id comparisons under the margin")
    return bad


def split_coverage(stats, split):
    """what a walk lacks of calls on both sides of an attention graph switch at position `split` (L2Z_ATTN_SPLIT_POS):
    l2z_transformer below and at or above it, a greedy and a sampled loop call that cross it in mid-call, and a loop call
    that starts at or above it"""
    done = [e for e in stats["log"] if "refusal" not in e and not e.get("skipped")]
    pos = [e["pos"] for e in done if e["op"] == "transformer"]
    loops = {k: [(e["pos"], min(e["pos"] + e["n"], stats["seq_len"])) for e in done if e["op"] == k] for k in ("greedy_run", "sample_run")}
    bad = []
    if not any(p < split for p in pos) or not any(p >= split for p in pos):
        bad.append(f"transformer at {sorted(pos)}: not on both sides of {split}")
    for k, v in loops.items():
        if not any(a < split < b for a, b in v):
            bad.append(f"no {k} call crosses {split}: {v}")
    if not any(a >= split for v in loops.values() for a, b in v):
        bad.append(f"no loop call starts at or above {split}")
    return bad
