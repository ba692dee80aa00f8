"""l2z_verify and what stands around it, without a GPU: the symbol is declared in the product header, listed in the version
script, exported by both libraries and bound in the Zig shim with the header's eight parameters; the two hooks are test-only;
the ABI version stays 2; the binding has RunState.verify, speculate_greedy and lookup_draft; the prompt-lookup drafter
follows its rule; the CLI lists --spec and refuses it where it does not apply before any device is touched; without a device
l2z_verify fails with L2Z_ERR_NO_DEVICE."""
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "llama2.zig_amd", "host")
EXE = os.path.join(HOST, "llama2")
HOOKS = ("l2z_verify_logits_read", "l2z_verify_time")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


def test_verify_is_declared_mapped_exported_and_bound(B):
    assert "l2z_verify" in B.declared_symbols("product")
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    assert "l2z_verify" in set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    assert "l2z_verify" in exported(B.PRODUCT_LIB_PATH)
    assert "l2z_verify" in exported(B.LIB_PATH)
    z = open(os.path.join(ROOT, "bindings", "zig", "llama2_hip.zig")).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(B.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"pub extern fn l2z_verify\(([^)]*)\)", z, flags=re.S)
    assert m, "llama2_hip.zig does not declare l2z_verify"
    h = re.search(r"\bl2z_verify\s*\(([^)]*)\)", hdr, flags=re.S)
    n_zig = len([a for a in m.group(1).split(",") if a.strip()])
    n_hdr = len([a for a in h.group(1).split(",") if a.strip()])
    assert n_zig == n_hdr == 8


def test_verify_hooks_are_test_only(B):
    for hook in HOOKS:
        assert hook in B.declared_symbols("test")
        assert hook not in B.declared_symbols("product")
        assert hook not in exported(B.PRODUCT_LIB_PATH)
        assert hook in exported(B.LIB_PATH)


def test_abi_version_is_still_2_with_verify(B):
    assert re.search(r"^#define L2Z_ABI_VERSION 2$", open(B.HEADER_PATH).read(), flags=re.M)
    assert B.lib().l2z_abi_version() == 2
    assert "l2z_verify" in B.declared_symbols("product")


def test_binding_has_verify_speculate_and_lookup(B):
    for name in ("verify", "verify_logits", "verify_time"):
        assert callable(getattr(B.RunState, name, None)), name
    assert callable(getattr(B, "speculate_greedy", None))
    assert callable(getattr(B, "lookup_draft", None))
    assert B.lib().l2z_verify.argtypes is not None and len(B.lib().l2z_verify.argtypes) == 8


def rule(history, k, max_ngram):
    """the drafter's rule, restated: longest n-gram first, the most recent earlier occurrence, what followed it"""
    h, n = list(history), len(history)
    for g in range(max_ngram, 0, -1):
        for j in range(n - g - 1, -1, -1):
            if h[j:j + g] == h[n - g:]:
                return h[j + g:min(j + g + k, n)]
    return []


def test_lookup_draft_follows_the_rule_on_random_histories(B):
    rng = np.random.default_rng(2718)
    n_hits = 0
    for case in range(400):
        n = int(rng.integers(0, 301)) if case % 8 else int(rng.integers(0, 6))
        hist = rng.integers(0, 4, size=n).astype(np.int32)
        k, g = int(rng.integers(1, 16)), int(rng.integers(1, 5))
        got = B.lookup_draft(hist, k, g).tolist()
        assert got == rule(hist.tolist(), k, g), (case, n, k, g)
        n_hits += bool(got)
    assert n_hits > 200
    # a large alphabet: mostly no hit, short n-grams
    for case in range(100):
        hist = rng.integers(0, 50, size=int(rng.integers(0, 120))).astype(np.int32)
        k, g = int(rng.integers(1, 16)), int(rng.integers(1, 5))
        assert B.lookup_draft(hist, k, g).tolist() == rule(hist.tolist(), k, g)


def test_lookup_draft_pinned_cases(B):
    ld = lambda h, k, g=3: B.lookup_draft(np.array(h, np.int32), k, g).tolist()
    assert ld([], 4) == []                                   # empty history
    assert ld([7], 4) == []
    assert ld([1, 2, 3, 4, 5, 6], 4) == []                   # no repeat
    assert ld([5, 9, 1, 5, 9, 2, 5, 9], 1, 2) == [2]         # the most recent of two matches wins
    assert ld([5, 9, 1, 5, 9, 2, 5, 9], 3, 2) == [2, 5, 9]
    # the 3-gram (1 2 3) occurred long ago, the 1-gram (3) again just now: the longer n-gram wins
    assert ld([1, 2, 3, 40, 8, 3, 50, 1, 2, 3], 2, 3) == [40, 8]
    assert ld([1, 2, 3, 40, 8, 3, 50, 1, 2, 3], 2, 1) == [50, 1]
    assert ld([4, 4], 8) == [4]                              # the draft stops at the end of the history
    assert ld([1, 2, 3, 1, 2], 15) == [3, 1, 2]
    assert ld([1, 2, 3, 4, 5, 6, 7, 8, 1, 2], 3) == [3, 4, 5]  # k caps it
    assert ld([1, 2, 3, 4, 5, 6, 7, 8, 1, 2], 15) == [3, 4, 5, 6, 7, 8, 1, 2]
    assert ld([1, 2, 1, 2], 0) == []
    assert ld([1, 2, 1, 2], 5) == [1, 2]                     # default max_ngram = 3 falls back to the 2-gram


def test_cli_lists_spec_and_refuses_what_does_not_combine(B):
    r = subprocess.run([EXE, "-h"], capture_output=True, text=True)
    assert "--spec" in r.stdout
    # (a.bin does not exist: a run that got as far as the checkpoint would say so instead)
    cases = [(["--spec", "4"], "-t 0"),                       # the default temperature is the reference's 1.0
             (["--spec", "4", "-t", "0.8"], "-t 0"),
             (["--spec", "4", "-t", "0", "-b", "2"], "--batch"),
             (["--spec", "4", "-t", "0", "-g", "2"], "--gpus"),
             (["--spec", "4", "-t", "0", "--score"], "--score"),
             (["--spec", "16", "-t", "0"], "0 to 15"),
             (["--spec", "-1", "-t", "0"], "0 to 15"),
             (["--spec", "x", "-t", "0"], "0 to 15")]
    for args, what in cases:
        r = subprocess.run([EXE, "a.bin", *args], capture_output=True, text=True)
        assert r.returncode != 0, args
        assert "--spec" in r.stderr and what in r.stderr, (args, r.stderr)
        assert "cannot open checkpoint" not in r.stderr, args
    r = subprocess.run([EXE, "a.bin", "--spec", "4", "-t", "0"], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot open checkpoint" in r.stderr   # accepted: got as far as the file


_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
B = ge.load_package().binding
L = B.lib()
tok = (C.c_int32 * 2)(1, 2)
out = (C.c_int32 * 2)(0, 0)
acc = C.c_int(0)
cfg = B.L2ZConfig(8, 16, 1, 2, 2, 10, 4)
print(L.l2z_verify(tok, 2, 0, C.byref(cfg), None, None, out, C.byref(acc)))
"""


def test_verify_without_a_device_returns_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    assert out.split() == [str(B.ERR_NO_DEVICE)], out
