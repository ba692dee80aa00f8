"""The tree form of the prompt-lookup drafter (l2zh_lookup_draft_tree, binding.lookup_draft_tree), host only: every earlier
occurrence of the history's last g tokens (g = max_ngram .. 1, most recent first) contributes its continuation; the
continuations are merged into a trie under a budget.  Guess k is tree node k + 1, parent[k] its parent's tree node."""
import numpy as np


def rule(hist, depth, budget, max_ngram):
    """a restatement of the rule in Python"""
    n = len(hist)
    tok, par = [], []
    if depth <= 0 or budget <= 0:
        return tok, par
    for g in range(max_ngram, 0, -1):
        if g + 1 > n:
            continue
        for j in range(n - g - 1, -1, -1):
            if hist[j:j + g] != hist[n - g:]:
                continue
            cur = 0
            for t in hist[j + g:j + g + depth]:
                child = next((c + 1 for c in range(len(tok)) if par[c] == cur and tok[c] == t), None)
                if child is None:
                    if len(tok) == budget:
                        return tok, par
                    tok.append(t); par.append(cur)
                    child = len(tok)
                cur = child
    return tok, par


def depths(par):
    d = [0]
    for p in par:
        d.append(d[p] + 1)
    return d


def check_shape(tok, par, depth, budget):
    assert len(tok) == len(par) <= budget
    for k, p in enumerate(par):
        assert 0 <= p <= k   # tree node k + 1 hangs below an earlier tree node
    assert max(depths(par)) <= depth
    keys = list(zip(par, tok))
    assert len(set(keys)) == len(keys)   # siblings carry different tokens


def test_tree_follows_the_rule_on_random_histories(B):
    rng = np.random.default_rng(3)
    seen_branching = 0
    for _ in range(300):
        n = int(rng.integers(0, 60))
        hist = rng.integers(0, 4, size=n).astype(np.int32)   # a small alphabet: many occurrences
        depth, budget, g = int(rng.integers(0, 7)), int(rng.integers(0, 16)), int(rng.integers(1, 4))
        tok, par = B.lookup_draft_tree(hist, depth, budget, g)
        assert (tok.tolist(), par.tolist()) == rule(hist.tolist(), depth, budget, g), (hist.tolist(), depth, budget, g)
        check_shape(tok.tolist(), par.tolist(), depth, budget)
        seen_branching += len(set(par.tolist())) < len(par)
        # deterministic
        tok2, par2 = B.lookup_draft_tree(hist, depth, budget, g)
        assert tok.tolist() == tok2.tolist() and par.tolist() == par2.tolist()
    assert seen_branching > 50


def test_the_first_branch_is_lookup_draft(B):
    rng = np.random.default_rng(4)
    for _ in range(200):
        hist = rng.integers(0, 5, size=int(rng.integers(1, 50))).astype(np.int32)
        depth, g = int(rng.integers(1, 8)), int(rng.integers(1, 4))
        chain = B.lookup_draft(hist, depth, g).tolist()
        tok, par = B.lookup_draft_tree(hist, depth, 15, g)
        assert tok[:len(chain)].tolist() == chain
        assert par[:len(chain)].tolist() == list(range(len(chain)))
        assert (len(tok) == 0) == (len(chain) == 0)


def test_two_continuations_of_the_last_token_both_appear(B):
    #        7 -> 3 4    ...    7 -> 5 6    ...    7
    hist = np.array([1, 7, 3, 4, 9, 7, 5, 6, 8, 7], np.int32)
    tok, par = B.lookup_draft_tree(hist, 2, 15, 3)
    assert tok.tolist() == [5, 6, 3, 4] and par.tolist() == [0, 1, 0, 3]   # the most recent occurrence first
    # a shared first token is ONE node with two children
    hist = np.array([1, 7, 3, 4, 9, 7, 3, 6, 8, 7], np.int32)
    tok, par = B.lookup_draft_tree(hist, 2, 15, 3)
    assert tok.tolist() == [3, 6, 4] and par.tolist() == [0, 1, 1]
    # the budget cuts the second branch, the depth every branch
    tok, par = B.lookup_draft_tree(np.array([1, 7, 3, 4, 9, 7, 5, 6, 8, 7], np.int32), 2, 3, 3)
    assert tok.tolist() == [5, 6, 3] and par.tolist() == [0, 1, 0]
    tok, par = B.lookup_draft_tree(np.array([1, 7, 3, 4, 9, 7, 5, 6, 8, 7], np.int32), 1, 15, 3)
    assert tok.tolist() == [5, 3] and par.tolist() == [0, 0]
    # a longer n-gram's occurrence comes before a more recent shorter one
    hist = np.array([2, 7, 3, 9, 7, 5, 2, 7], np.int32)
    tok, par = B.lookup_draft_tree(hist, 1, 15, 2)
    assert tok.tolist() == [3, 5] and par.tolist() == [0, 0]


def test_no_match_gives_no_nodes(B):
    for hist in ([], [5], [1, 2, 3, 4]):
        tok, par = B.lookup_draft_tree(np.array(hist, np.int32), 4, 15, 3)
        assert len(tok) == 0 and len(par) == 0
    hist = np.array([1, 7, 3, 7], np.int32)
    assert len(B.lookup_draft_tree(hist, 0, 15)[0]) == 0
    assert len(B.lookup_draft_tree(hist, 4, 0)[0]) == 0
    assert B.lookup_draft_tree(hist, 4, 40)[0].tolist() == [3, 7]   # (a budget above 15 is 15)
