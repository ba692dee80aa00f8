"""The single-sequence speculation loops of the binding (speculate_greedy, speculate_sample, speculate_q8, speculate_tree),
without a GPU: over a fixed grid, the ids and stats they return and EVERY call they make on the runstate -- method, tokens,
parents, position, and the draw arguments exactly as passed or absent -- are those of a record, tests/golden/
speculate_loops.json.  The model is replaced by an explicit arithmetic hash of (history, coin), so the record does not
depend on the interpreter, and the drafters are functions of the history alone.

How the record is made: this same file, run in a checkout of the commit to record with the switch set to a name for it,

    L2Z_RECORD_SPECULATE_LOOPS=<commit id> python -m pytest tests/test_speculate_loops_cpu.py

writes the file instead of comparing (and says which commit it was made from in "made_from").  The committed record was
made from cc43edf, the last commit in which each of the four functions had a loop of its own; it is remade only when a
change means to alter what the loops call."""
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "speculate_loops.json")
RECORD = os.environ.get("L2Z_RECORD_SPECULATE_LOOPS")

VOCAB, STEPS, PROMPT = 50, 20, [5, 6, 7]
T, P = 0.8, 0.9


def bits(coin) -> int:
    return int(np.asarray(coin, np.float32).reshape(-1)[0:1].view(np.uint32)[0])


def mix(history, coin) -> int:
    """FNV-1a over the history's ids and the coin's f32 bits, then one xor-shift: 32 bits"""
    h = 2166136261
    for v in [int(t) for t in history] + [bits(coin) & 0xFFFF, bits(coin) >> 16]:
        h = ((h ^ v) * 16777619) & 0xFFFFFFFF
    return h ^ (h >> 15)


class Fake:
    """A runstate as the loops see it.  The id after a history is a function of the history and the coin it is drawn with
    (greedy: coin 0): never BOS, except -- bos_at -- after the history of that length.  Every call is logged."""

    def __init__(self, B, seq_len, bos_at=None):
        self.cfg, self.seen, self.log, self.bos_at = B.L2ZConfig(8, 16, 1, 2, 2, VOCAB, seq_len), [], [], bos_at

    def draw(self, history, coin):
        return 1 if len(history) == self.bos_at else 2 + mix(history, coin) % (VOCAB - 2)

    @staticmethod
    def passed(args):
        """the draw arguments of a call as they came: temperature, top_p, the coins' f32 bits"""
        return [a if not hasattr(a, "__len__") else [bits(c) for c in a] for a in args]

    def _prefill(self, name, tokens, pos0):
        self.log.append([name, [int(t) for t in tokens], pos0])
        self.seen = [int(t) for t in tokens]

    def prefill(self, tokens, pos0, w):
        self._prefill("prefill", tokens, pos0)

    def prefill_q8(self, tokens, pos0, w):
        self._prefill("prefill_q8", tokens, pos0)

    def argmax(self):
        self.log.append(["argmax"])
        return self.draw(self.seen, 0.0)

    def sample_first(self, temperature, top_p, coin):
        self.log.append(["sample_batch", temperature, top_p, bits(coin)])
        return self.draw(self.seen, coin)

    def _tree(self, tokens, parent, pos0, coins):
        """l2z_verify_tree's contract on the hash (a chain: parent i - 1)"""
        assert pos0 == len(self.seen) and parent[0] == -1 and len(tokens) <= 16
        dep, hist, nxt = [0], [self.seen + [int(tokens[0])]], []
        for i in range(1, len(tokens)):
            assert 0 <= parent[i] < i
            dep.append(dep[parent[i]] + 1)
            hist.append(hist[parent[i]] + [int(tokens[i])])
        assert pos0 + max(dep) < self.cfg.seq_len, "a row beyond the cache"
        assert coins is None or len(coins) == max(dep) + 1, "one coin per depth"
        for i in range(len(tokens)):
            nxt.append(self.draw(hist[i], 0.0 if coins is None else coins[dep[i]]))
        path = [0]
        while True:
            kids = [i for i in range(1, len(tokens)) if parent[i] == path[-1] and int(tokens[i]) == nxt[path[-1]]]
            if not kids:
                break
            path.append(kids[0])
        self.seen = hist[path[-1]]
        return np.array(nxt, np.int32), np.array(path, np.int32), len(path) - 1

    def _chain(self, tokens, pos0, coins):
        nxt, _, a = self._tree(tokens, list(range(-1, len(tokens) - 1)), pos0, coins)
        return nxt, a

    def verify(self, tokens, pos0, w):
        self.log.append(["verify", [int(t) for t in tokens], pos0])
        return self._chain(tokens, pos0, None)

    def verify_sample(self, tokens, pos0, w, temperature, top_p, coins):
        self.log.append(["verify_sample", [int(t) for t in tokens], pos0] + self.passed([temperature, top_p, coins]))
        return self._chain(tokens, pos0, coins)

    def verify_q8(self, tokens, pos0, w, *draw):
        self.log.append(["verify_q8", [int(t) for t in tokens], pos0] + self.passed(draw))
        return self._chain(tokens, pos0, draw[2] if draw else None)

    def verify_tree(self, tokens, parent, pos0, w, *draw):
        self.log.append(["verify_tree", [int(t) for t in tokens], [int(p) for p in parent], pos0] + self.passed(draw))
        return self._tree(tokens, parent, pos0, draw[2] if draw else None)


def wrong(ids):
    return (np.asarray(ids, np.int64) - 2 + 1) % (VOCAB - 2) + 2


def chain_drafters(full):
    """drafter(history, k) by name, `full` = BOS + the ids of the run"""
    rng = np.random.default_rng(3)
    full = np.asarray(full, np.int64)

    def truth(h, k):
        return full[len(h):len(h) + k]

    def half_wrong(h, k):
        g = truth(h, k).copy()
        bad = rng.random(len(g)) < 0.5
        g[bad] = wrong(g[bad])
        return g

    return {"truth": truth, "half_wrong": half_wrong, "two_short": lambda h, k: truth(h, max(0, k - 2)),
            "all_wrong": lambda h, k: wrong(truth(h, k)), "lookup": None}


def tree_drafters(full):
    """drafter(history, depth, budget) -> (tokens, parent) in lookup_draft_tree's convention, by name"""
    full = np.asarray(full, np.int64)

    def chain(h, d, b):
        t = full[len(h):len(h) + d][:b]
        return t, np.arange(len(t))

    def branches(h, d, b):   # at every depth a wrong sibling stands in front of the right id
        tok, par, at = [], [], 0
        for t in full[len(h):len(h) + d]:
            tok += [int(wrong(t)), int(t)]
            par += [at, at]
            at = len(tok)
        return np.array(tok[:b], np.int64), np.array(par[:b], np.int64)

    def oversize(h, d, b):   # two levels deeper than asked, b siblings too many, and guesses behind dropped nodes
        tok = [int(t) for t in full[len(h):len(h) + d + 2]]
        par = list(range(len(tok)))
        deep = len(tok)               # the deepest node of the chain: dropped wherever the chain is longer than d
        tok.append(3); par.append(deep)
        for j in range(b + 2):
            tok.append(2 + j % 5); par.append(0)
        tok.append(4); par.append(len(tok) - 1)   # behind the last sibling, which the budget has dropped
        return np.array(tok, np.int64), np.array(par, np.int64)

    return {"chain": chain, "branches": branches, "oversize": oversize, "lookup": None}


def grid(B, monkeypatch):
    """every run of the grid by name -> {"tokens", "stats", "log"}, a refusal -> {"error": its message}"""
    monkeypatch.setattr(B, "sample_batch", lambda states, t, p, c: np.array([states[0].sample_first(t, p, c)], np.int32))
    coins = B.coin_stream(12, STEPS)
    runs = {}

    def run(name, fn, *args, seq_len=64, bos_at=None):
        s = Fake(B, seq_len, bos_at)
        toks, stats = fn(s, None, *args)
        assert toks.dtype == np.int32
        runs[name] = {"tokens": toks.tolist(), "stats": stats, "log": s.log}
        return runs[name]

    # the four loops; `draw`: what follows the drafter in the arguments
    chains = {"greedy": (B.speculate_greedy, None), "sample": (B.speculate_sample, (T, P, coins)),
              "q8": (B.speculate_q8, ()), "q8_sampled": (B.speculate_q8, (T, P, coins))}

    def chain_call(mode, prompt, steps, k, drafter, **kw):
        fn, draw = chains[mode]
        if mode == "sample":   # (its drafter comes last)
            return lambda name: run(name, fn, prompt, steps, k, *draw, drafter, **kw)
        return lambda name: run(name, fn, prompt, steps, k, drafter, *(draw or ()), **kw)

    trees = {"tree": (), "tree_sampled": (T, None, coins)}   # (top_p None: the default)

    for mode in chains:
        base = chain_call(mode, PROMPT, STEPS, 0, None)(f"{mode} k=0")
        full = [1] + base["tokens"]
        for k in (1, 4, 15):
            for dn, d in chain_drafters(full).items():
                chain_call(mode, PROMPT, STEPS, k, d)(f"{mode} k={k} {dn}")
        truth = chain_drafters(full)["truth"]
        # n_steps = 0 on a short cache: the last call is clipped at its end (the ids are the base's: same hash)
        chain_call(mode, PROMPT, 0, 15, truth, seq_len=STEPS)(f"{mode} to the cache's end")
        chain_call(mode, [5, 6, 7, 8, 9, 10], 4, 4, truth)(f"{mode} prompt longer than n_steps")
        chain_call(mode, [5, 1, 7], STEPS, 4, truth)(f"{mode} BOS in the prompt")
        bos = chain_call(mode, PROMPT, STEPS, 0, None, bos_at=11)(f"{mode} BOS k=0")
        chain_call(mode, PROMPT, STEPS, 4, chain_drafters([1] + bos["tokens"])["truth"], bos_at=11)(f"{mode} BOS k=4 truth")
    for mode, draw in trees.items():
        fn = B.speculate_tree
        base = run(f"{mode} 0/0", fn, PROMPT, STEPS, 0, 0, None, *draw)
        full = [1] + base["tokens"]
        for depth, budget in ((0, 4), (4, 0), (1, 1), (4, 4), (4, 15), (15, 4), (15, 15)):
            for dn, d in tree_drafters(full).items():
                run(f"{mode} {depth}/{budget} {dn}", fn, PROMPT, STEPS, depth, budget, d, *draw)
        td = tree_drafters(full)
        run(f"{mode} to the cache's end", fn, PROMPT, 0, 15, 15, td["branches"], *draw, seq_len=STEPS)
        run(f"{mode} prompt longer than n_steps", fn, [5, 6, 7, 8, 9, 10], 4, 4, 4, td["chain"], *draw)
        run(f"{mode} BOS in the prompt", fn, [5, 1, 7], STEPS, 4, 4, td["chain"], *draw)
        bos = run(f"{mode} BOS 0/0", fn, PROMPT, STEPS, 0, 0, None, *draw, bos_at=11)
        run(f"{mode} BOS 4/8 branches", fn, PROMPT, STEPS, 4, 8, tree_drafters([1] + bos["tokens"])["branches"], *draw, bos_at=11)

    # refusals: the range of k / budget first, then the coins; none of them reaches the runstate
    class Bare:   # (any call on it would be an AttributeError)
        cfg = B.L2ZConfig(8, 16, 1, 2, 2, VOCAB, 12)

    def refuse(name, fn, *args):
        try:
            fn(Bare(), None, *args)
            runs[name] = {"error": None}
        except ValueError as e:
            runs[name] = {"error": str(e)}

    z = lambda n: np.zeros(n, np.float32)
    for k in (16, -1):
        refuse(f"greedy refuses k={k}", B.speculate_greedy, [3, 4], 0, k)
        refuse(f"sample refuses k={k}", B.speculate_sample, [3, 4], 0, k, 1.0, 0.9, z(64))
        refuse(f"sample refuses k={k} before the coins", B.speculate_sample, [3, 4], 0, k, 1.0, 0.9, z(1))
        refuse(f"q8 refuses k={k}", B.speculate_q8, [3, 4], 0, k)
        refuse(f"q8 refuses k={k} before the coins", B.speculate_q8, [3, 4], 0, k, None, 1.0, 0.9, z(1))
        refuse(f"tree refuses budget={k}", B.speculate_tree, [3, 4], 0, 4, k)
        refuse(f"tree refuses budget={k} before the coins", B.speculate_tree, [3, 4], 0, 4, k, None, 1.0, 0.9, z(1))
    for n_steps, n in ((0, 9), (8, 5)):   # 12 or 8 positions, 2 of them the prompt's: one coin short
        refuse(f"sample refuses {n} coins for n_steps={n_steps}", B.speculate_sample, [3, 4], n_steps, 4, 1.0, 0.9, z(n))
        refuse(f"q8 refuses {n} coins for n_steps={n_steps}", B.speculate_q8, [3, 4], n_steps, 4, None, 1.0, 0.9, z(n))
        refuse(f"tree refuses {n} coins for n_steps={n_steps}", B.speculate_tree, [3, 4], n_steps, 4, 4, None, 1.0, 0.9, z(n))
    return json.loads(json.dumps(runs))


def test_speculation_loops_call_the_runstate_as_recorded(B, monkeypatch):
    got = grid(B, monkeypatch)
    # what the grid is there to reach, whatever the record says
    assert all(r["error"] for n, r in got.items() if "refuses" in n)
    for mode in ("greedy", "sample", "q8", "q8_sampled", "tree", "tree_sampled"):
        base = got[f"{mode} k=0" if "tree" not in mode else f"{mode} 0/0"]
        assert len(base["tokens"]) == STEPS and base["stats"]["offered"] == 0
        same = [n for n in got if n.startswith(mode + " ") and ("k=" in n or "/" in n) and "BOS" not in n and "refuses" not in n]
        assert len(same) >= 16 and all(got[n]["tokens"] == base["tokens"] for n in same), mode   # draft invariance
        assert got[f"{mode} to the cache's end"]["tokens"] == base["tokens"]   # (the fake refuses a row beyond the cache)
        none = dict(calls=0, offered=0, accepted=0, emitted=0)
        assert got[f"{mode} prompt longer than n_steps"] == {"tokens": [5, 6, 7, 8], "stats": none, "log": []}
        assert got[f"{mode} BOS in the prompt"] == {"tokens": [5, 1], "stats": none, "log": []}
        ended = got[f"{mode} BOS k=4 truth" if "tree" not in mode else f"{mode} BOS 4/8 branches"]["stats"]
        assert ended["emitted"] < ended["calls"] + ended["accepted"], mode   # the BOS was not the last id of its call
    if RECORD:
        with open(GOLDEN, "w") as f:
            json.dump({"made_from": RECORD, "runs": got}, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
        return
    want = json.load(open(GOLDEN))["runs"]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
