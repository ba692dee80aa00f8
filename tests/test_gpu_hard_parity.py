"""Every forward-pass family on the GPU against the float64 model on HARD checkpoints (tests/hard_models.py, DESIGN.md "Hard
checkpoints"): a flat attention whose weights are exactly 1 / (pos + 1), a peaked one, one whose exponentials underflow to
0, and one with a few outlier channels -- the statistics on which the max subtraction, the online rescale of the segment and
split combines, the `weight > 0` skip of the verify family's V sweep, the flash kernels' running maximum and the three-term
bf16 split do work that `synth_blob` weights never ask of them.

Every call is arranged so that each row it produces is some position p of the case's ONE token chain T, and every row is
held to

    max |gpu - z64[p]| <= bar[p] = LOGIT_ATOL + FACTOR * D[p]

with z64 the float64 logits and D[p] the distance of the reference's own twelve fp32 readings from them (nothing in the bar
comes from a GPU); the emitted id must be the float64 model's wherever its top-2 margin exceeds 2 * bar[p], and at most 5 %
of a test's rows may fall under that rule.  A test checks all its rows, prints its worst err / bar and err / D
(profiles/hard_parity.md records them) and then fails on any row over its bar.

Each case has one world: the blob uploaded, a base runstate holding T[:L - 1], and forks of it at the depths a test needs.
"""
import numpy as np
import pytest

import hard_models as hm
from test_gpu_prefill_batch import bits
from test_gpu_wide_decode import forked

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("case", hm.CASES, ids=hm.CASE_IDS)
X3 = pytest.mark.parametrize("x3", [1, 2], ids=["x3_1", "x3_2"])
# (family, L2Z_PF_X3) -> the bar's factor where 4 is short for a sound piece of arithmetic (DESIGN.md names the step);
# empty: every family holds the factor of test_gpu_inside_reference_spread
FACTORS = {}


def SLICES(L):
    """(pos0, rows) of the prompt slices: 64 and 65 rows from 0, one across 64 and 128, one ending on seq_len - 1, one inside"""
    return [(0, 64), (0, 65), (60, 70), (L - 9, 9), (10, 33)]


class World:
    """a case on the GPU: the blob uploaded, the chain's first seq_len - 1 tokens in a base runstate, forks of it"""

    def __init__(self, gpu, ref):
        self.gpu, self.ref, self.cfg = gpu, ref, ref.cfg
        self.L = ref.cfg.seq_len
        self.T = ref.T
        self.w = gpu.Weights(ref.cfg, ref.blob, False)
        self.base = gpu.RunState(ref.cfg)
        self.base.prefill(self.T[:self.L - 1], 0, self.w)
        self.base.synchronize()
        self._garbage = None

    def garbage(self):
        """a runstate whose every cache row holds another sequence's contents"""
        if self._garbage is None:
            rng = np.random.default_rng([hm.SEED, 8])
            self._garbage = self.gpu.RunState(self.cfg)
            self._garbage.prefill(rng.integers(2, self.cfg.vocab_size, self.L).astype(np.int32), 0, self.w)
            self._garbage.synchronize()
        return self._garbage

    def fork(self, depths, garbage=None, pool=None):
        if pool is None:
            return [forked(self.gpu, self.base, int(d), garbage) for d in depths]
        out = []
        for d in depths:
            s = self.gpu.RunState(self.cfg, pool=pool)
            self.gpu.runstate_fork(s, self.base, int(d))
            s.synchronize()
            out.append(s)
        return out

    def depths(self, n, salt, hi=None):
        """n depths: seq_len - 1 and the segment edges first, then drawn ones (below hi)"""
        rng = np.random.default_rng([hm.SEED, 6, salt])
        edges = [self.L - 1] + list(hm.EDGES)
        return np.array(edges + rng.integers(0, hi or self.L, n - len(edges)).tolist(), np.int32)

    def close(self):
        for s in (self.base, self._garbage):
            if s is not None:
                s.close()
        self.w.close()


@pytest.fixture(scope="module")
def worlds(gpu, ck, orc):
    made = {}

    def get(case):
        if case not in made:
            made[case] = World(gpu, hm.reference(ck, orc, *case))
        return made[case]
    yield get
    for wd in made.values():
        wd.close()


def close(*groups):
    for g in groups:
        for s in g:
            s.close()


class Tally:
    """a test's rows against the reference: every row is measured, finish() prints the worst ratios and then asserts"""

    def __init__(self, ref, family, x3=None):
        self.ref, self.family, self.x3 = ref, family, x3
        self.factor = FACTORS.get((family, x3), hm.FACTOR)
        self.bar = hm.LOGIT_ATOL + self.factor * ref.D
        self.rows = self.under = 0
        self.worst_bar = self.worst_d = 0.0
        self.at = None
        self.bad = []

    def value(self, what, p, err, scale=1):
        """one row's distance `err` from the float64 model, held to scale * bar[p]"""
        r = err / (scale * self.bar[p])
        if not r <= self.worst_bar:
            self.worst_bar, self.at = r, (what, p)
        self.worst_d = max(self.worst_d, err / (scale * self.ref.D[p])) if np.isfinite(err) else float("inf")
        if not err <= scale * self.bar[p]:
            self.bad.append((what, p, err, scale * float(self.bar[p])))

    def token(self, what, p, emitted):
        """the id emitted for position p, under the margin rule"""
        if self.ref.margin[p] > 2 * self.bar[p]:
            if int(emitted) != int(self.ref.top[p]):
                self.bad.append((what, p, "id", int(emitted), int(self.ref.top[p])))
        else:
            self.under += 1

    def row(self, what, p, logits, emitted=None):
        p = int(p)
        self.rows += 1
        self.value(what, p, float(np.abs(logits.astype(np.float64) - self.ref.z64[p]).max()))
        if emitted is not None:
            self.token(what, p, emitted)

    def finish(self):
        x3 = "" if self.x3 is None else f" x3={self.x3}"
        print(f"HARD {self.family} {self.ref.shape}-{self.ref.kind}{x3}: rows {self.rows} worst err/bar {self.worst_bar:.3f} "
              f"at {self.at} worst err/D {self.worst_d:.3f} under the margin rule {self.under} factor {self.factor}")
        assert not self.bad, (len(self.bad), self.bad[:8])
        assert self.under <= 0.05 * self.rows, "vacuous: too many rows left out of the token comparison"


# ---- stepped decode ----
@CASES
def test_stepped_decode_and_the_split_attention(gpu, worlds, options, case):
    """l2z_transformer at p = 0 .. L - 1 with the attention form the position picks, then with the split (flash-decoding)
    attention forced at every position: 3 chunks per head (positions below 3 leave chunks empty) and 16"""
    wd = worlds(case)
    for nch in (-1, 3, 16):
        options(L2Z_ATTN_SPLIT=nch)   # read when a runstate is made
        s = gpu.RunState(wd.cfg)
        t = Tally(wd.ref, "stepped" if nch < 0 else f"stepped-split{nch}")
        for p in range(wd.L):
            s.transformer(int(wd.T[p]), p, wd.w)
            t.row("step", p, s.logits(), s.argmax())
        s.close()
        t.finish()


# ---- prompt passes ----
@X3
@CASES
def test_prefill(gpu, worlds, options, case, x3):
    """l2z_prefill of T[:n]: one, two and three query tiles, both sides of the 64-row edge, the whole context"""
    wd = worlds(case)   # (made under the default options)
    options(L2Z_PF_X3=x3)
    t = Tally(wd.ref, "prefill", x3)
    s = gpu.RunState(wd.cfg)
    for n in (17, 64, 65, 129, wd.L):
        s.prefill(wd.T[:n], 0, wd.w)
        t.row(f"prefill {n}", n - 1, s.logits(), s.argmax())
    s.close()
    t.finish()


@X3
@CASES
def test_score(gpu, worlds, options, case, x3):
    """l2z_score(T): every position's log-prob of the chain's next token against the float64 log_softmax within 2 * bar[p]
    (a log-prob is a logit less the log-sum-exp, and either moves by at most max |dz|); top-1 under the margin rule"""
    wd = worlds(case)   # (made under the default options)
    options(L2Z_PF_X3=x3)
    t = Tally(wd.ref, "score", x3)
    s = gpu.RunState(wd.cfg)
    lp, top = s.score(wd.T, 0, wd.w)
    want = hm.log_softmax64(wd.ref.z64)
    for p in range(wd.L):
        t.rows += 1
        if p < wd.L - 1:
            t.value("score", p, abs(float(lp[p]) - float(want[p, wd.T[p + 1]])), scale=2)
        t.token("score", p, top[p])
    assert lp[wd.L - 1] == 0.0   # no target behind the last position
    s.close()
    t.finish()


@X3
@CASES
def test_prefill_batch(gpu, worlds, options, case, x3):
    """l2z_prefill_batch on slices of the chain, each on a fork at its first position; every sequence's last row"""
    wd = worlds(case)   # (made under the default options)
    options(L2Z_PF_X3=x3)
    lay = SLICES(wd.L)
    t = Tally(wd.ref, "prefill_batch", x3)
    states = wd.fork([p for p, _ in lay])
    gpu.prefill_batch(states, [wd.T[p:p + r] for p, r in lay], [p for p, _ in lay], wd.w)
    ids = gpu.argmax_batch(states)
    for s, (p, r), i in zip(states, lay, ids):
        t.row(f"slice {p}+{r}", p + r - 1, s.logits(), i)
    close(states)
    t.finish()


# ---- batched step ----
@CASES
def test_batched_step(gpu, worlds, case):
    """l2z_transformer_batch, 16 forks"""
    wd = worlds(case)
    t = Tally(wd.ref, "batch16")
    d = wd.depths(16, 1)
    states = wd.fork(d)
    gpu.transformer_batch(states, wd.T[d], d, wd.w)
    ids = gpu.argmax_batch(states)
    for s, p, i in zip(states, d, ids):
        t.row("batch", p, s.logits(), i)
    close(states)
    t.finish()


# ---- verify family ----
def verify_p0s(L):
    return (0, 56, 120, L - 16)


@X3
@CASES
def test_verify_and_verify_sample(gpu, worlds, options, case, x3):
    """l2z_verify on T[p0 : p0 + 16], and l2z_verify_sample the same at temperature 0: every guess is the chain's own
    token, so every row is a chain position (rows through l2z_verify_logits_read)"""
    wd = worlds(case)   # (made under the default options)
    options(L2Z_PF_X3=x3)
    for fam in ("verify", "verify_sample"):
        t = Tally(wd.ref, fam, x3)
        for p0 in verify_p0s(wd.L):
            s, = wd.fork([p0])
            toks = wd.T[p0:p0 + 16]
            nxt, acc = s.verify(toks, p0, wd.w) if fam == "verify" else s.verify_sample(toks, p0, wd.w, 0.0, 1.0, None)
            assert 0 <= acc <= 15
            for i in range(16):
                t.row(f"{fam} {p0}", p0 + i, s.verify_logits(i), nxt[i])
            s.close()
        t.finish()


@X3
@CASES
def test_verify_batch(gpu, worlds, options, case, x3):
    """l2z_verify_batch: 4 sequences of 4 rows, across positions 64 and 128 and up to the context's end"""
    wd = worlds(case)   # (made under the default options)
    options(L2Z_PF_X3=x3)
    t = Tally(wd.ref, "verify_batch", x3)
    p0s = [0, 62, 126, wd.L - 4]
    states = wd.fork(p0s)
    nxts, acc = gpu.verify_batch(states, [wd.T[p:p + 4] for p in p0s], p0s, wd.w)
    for j, p0 in enumerate(p0s):
        for i in range(4):
            t.row(f"verify_batch {p0}", p0 + i, states[0].verify_logits(4 * j + i), nxts[j][i])
    close(states)
    t.finish()


@X3
@CASES
def test_verify_tree(gpu, worlds, options, case, x3):
    """l2z_verify_tree: the chain T[60:68] with one wrong sibling under each of its first seven nodes, 15 nodes.  The
    chain's rows against z64, out_next on the chain under the margin rule; the verdict walks the chain."""
    wd = worlds(case)   # (made under the default options)
    options(L2Z_PF_X3=x3)
    V, p0 = wd.cfg.vocab_size, 60
    toks, parent, chain = [int(wd.T[p0])], [-1], [0]
    for d in range(1, 8):
        right = int(wd.T[p0 + d])
        wrong = 2 + (right - 2 + 1) % (V - 2)
        assert wrong != right and 2 <= wrong < V
        toks += [right, wrong]
        parent += [chain[-1], chain[-1]]
        chain.append(len(toks) - 2)
    assert len(toks) == 15
    t = Tally(wd.ref, "verify_tree", x3)
    s, = wd.fork([p0])
    nxt, path, acc = s.verify_tree(toks, parent, p0, wd.w)
    for d, node in enumerate(chain):
        t.row("tree", p0 + d, s.verify_logits(node), nxt[node])
    s.close()
    t.finish()
    walk = [0]   # the verdict's rule on the ids the call returned: on to the child that holds the parent's next token
    while True:
        kids = [c for c in range(len(toks)) if parent[c] == walk[-1] and toks[c] == int(nxt[walk[-1]])]
        if not kids:
            break
        walk.append(kids[0])
    assert path.tolist() == walk and acc == len(walk) - 1


# ---- wide family ----
@X3
@CASES
def test_wide_step(gpu, worlds, options, case, x3):
    """l2z_transformer_wide at 33 and 128 rows (a step rewrites row pos[i] before anything reads it, so the 128 forks
    serve both)"""
    wd = worlds(case)   # (made under the default options)
    options(L2Z_PF_X3=x3)
    d = wd.depths(128, 2)
    states = wd.fork(d)
    for n in (33, 128):
        t = Tally(wd.ref, f"wide{n}", x3)
        nxt = gpu.transformer_wide(states[:n], wd.T[d[:n]], d[:n], wd.w)
        for i in range(n):
            t.row(f"wide {n}", d[i], states[i].logits(), nxt[i])
        t.finish()
    close(states)


@X3
@CASES
def test_verify_wide(gpu, worlds, options, case, x3):
    """l2z_verify_wide: 8 sequences of 16 rows"""
    wd = worlds(case)   # (made under the default options)
    options(L2Z_PF_X3=x3)
    rng = np.random.default_rng([hm.SEED, 6, 3])
    p0s = list(verify_p0s(wd.L)) + rng.integers(0, wd.L - 15, 4).tolist()
    t = Tally(wd.ref, "verify_wide", x3)
    states = wd.fork(p0s)
    nxts, acc = gpu.verify_wide(states, [wd.T[p:p + 16] for p in p0s], p0s, wd.w)
    for j, p0 in enumerate(p0s):
        for i in range(16):
            t.row(f"verify_wide {p0}", p0 + i, states[0].verify_logits(16 * j + i), nxts[j][i])
    close(states)
    t.finish()


def mixed_layout(wd):
    """the five prompt slices, then one-row sequences at the seven edge depths and 20 drawn ones"""
    lay = SLICES(wd.L) + [(int(p), 1) for p in wd.depths(27, 4)]
    assert len(lay) == 32 and sum(r for _, r in lay) == 241 + 27
    return lay


@X3
@CASES
def test_step_mixed(gpu, worlds, options, case, x3):
    """l2z_step_mixed: prompt slices and decode rows in one sweep; every sequence's last row"""
    wd = worlds(case)   # (made under the default options)
    options(L2Z_PF_X3=x3)
    lay = mixed_layout(wd)
    t = Tally(wd.ref, "step_mixed", x3)
    states = wd.fork([p for p, _ in lay])
    nxt = gpu.step_mixed(states, [wd.T[p:p + r] for p, r in lay], [p for p, _ in lay], wd.w)
    for s, (p, r), i in zip(states, lay, nxt):
        t.row(f"mixed {p}+{r}", p + r - 1, s.logits(), i)
    close(states)
    t.finish()


@X3
def test_paged_runstates_give_the_same_bits(gpu, worlds, options, x3):
    """one l2z_step_mixed and one l2z_transformer_wide call of the tests above on paged runstates: bit-equal logits and ids"""
    wd = worlds(("kvmul3", "onehot"))   # (made under the default options)
    options(L2Z_PF_X3=x3)
    lay = mixed_layout(wd)
    d = wd.depths(33, 2)

    def pages(ends):
        return sum((int(e) + 63) // 64 for e in ends)
    pool = gpu.KvPool(wd.cfg, pages([p + r for p, r in lay]) + pages(d + 1))
    got = {}
    for kind in ("contiguous", "paged"):
        pl = pool if kind == "paged" else None
        a, b = wd.fork([p for p, _ in lay], pool=pl), wd.fork(d, pool=pl)
        ids_a = gpu.step_mixed(a, [wd.T[p:p + r] for p, r in lay], [p for p, _ in lay], wd.w)
        ids_b = gpu.transformer_wide(b, wd.T[d], d, wd.w)
        got[kind] = (ids_a, ids_b, [bits(s.logits()) for s in a + b])
        close(a, b)
    assert pool.info()["n_free"] == pool.info()["n_pages"]
    pool.close()
    assert np.array_equal(got["paged"][0], got["contiguous"][0]) and np.array_equal(got["paged"][1], got["contiguous"][1])
    for i, (x, y) in enumerate(zip(got["paged"][2], got["contiguous"][2])):
        assert np.array_equal(x, y), i


# ---- flat: stale rows cannot hide ----
@X3
@pytest.mark.parametrize("shape", ["kvmul3", "hs64h"])
def test_flat_stale_rows_are_never_read(gpu, worlds, options, shape, x3):
    """On `flat` every key of a context weighs exactly 1 / (pos + 1), so a stale row that was read -- or a live one that
    was not -- moves the output by a whole share.  After l2z_prefill_batch on the slices and after three
    l2z_transformer_wide steps, runstates forked over a cache full of another sequence's rows must hold the logits, bit for
    bit, of runstates forked over zeros; the third step's logits against z64 as well."""
    wd = worlds((shape, "flat"))   # (made under the default options)
    options(L2Z_PF_X3=x3)
    lay = SLICES(wd.L)
    d = np.minimum(wd.depths(33, 5), wd.L - 3).astype(np.int32)
    t = Tally(wd.ref, "flat-stale", x3)
    got = {}
    for kind in ("clean", "garbage"):
        g = wd.garbage() if kind == "garbage" else None
        a, b = wd.fork([p for p, _ in lay], garbage=g), wd.fork(d, garbage=g)
        gpu.prefill_batch(a, [wd.T[p:p + r] for p, r in lay], [p for p, _ in lay], wd.w)
        for k in range(3):
            nxt = gpu.transformer_wide(b, wd.T[d + k], d + k, wd.w)
        if kind == "garbage":
            for s, (p, r) in zip(a, lay):
                t.row(f"slice {p}+{r}", p + r - 1, s.logits())
            for i, s in enumerate(b):
                t.row("third wide step", d[i] + 2, s.logits(), nxt[i])
        got[kind] = [bits(s.logits()) for s in a + b]
        close(a, b)
    for i, (x, y) in enumerate(zip(got["garbage"], got["clean"])):
        assert np.array_equal(x, y), (shape, "stale rows changed sequence", i)
    t.finish()
