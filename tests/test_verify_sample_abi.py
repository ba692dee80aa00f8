"""l2z_verify_sample and what stands around it, without a GPU: the symbol is declared in the product header, listed in the
version script, exported by both libraries and bound in the Zig shim with the header's eleven parameters; the timing hook is
test-only; the ABI version stays 2 and the product library exports the header's 31 functions; the binding has
RunState.verify_sample, speculate_sample and coin_stream, and coin_stream is l2zh_prng_floats; the CLI lists --spec-sample,
refuses it where it does not apply before any file or device is touched and accepts it at the default temperature; without a
device l2z_verify_sample fails with L2Z_ERR_NO_DEVICE."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "llama2.zig_amd", "host")
EXE = os.path.join(HOST, "llama2")
NAME = "l2z_verify_sample"
HOOK = "l2z_verify_sample_time"


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


def test_verify_sample_is_declared_mapped_exported_and_bound(B):
    assert NAME in B.declared_symbols("product")
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    assert NAME in set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    assert NAME in exported(B.PRODUCT_LIB_PATH)
    assert NAME in exported(B.LIB_PATH)
    z = open(os.path.join(ROOT, "bindings", "zig", "llama2_hip.zig")).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(B.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"pub extern fn l2z_verify_sample\(([^)]*)\)", z, flags=re.S)
    assert m, "llama2_hip.zig does not declare l2z_verify_sample"
    h = re.search(r"\bl2z_verify_sample\s*\(([^)]*)\)", hdr, flags=re.S)
    n_zig = len([a for a in m.group(1).split(",") if a.strip()])
    n_hdr = len([a for a in h.group(1).split(",") if a.strip()])
    assert n_zig == n_hdr == 11


def test_product_library_exports_the_headers_31_functions(B):
    declared = set(B.declared_symbols("product"))
    assert len(declared) == 31
    assert {n for n in exported(B.PRODUCT_LIB_PATH) if n.startswith("l2z_")} == declared


def test_verify_sample_hook_is_test_only(B):
    assert HOOK in B.declared_symbols("test")
    assert HOOK not in B.declared_symbols("product")
    assert HOOK not in exported(B.PRODUCT_LIB_PATH)
    assert HOOK in exported(B.LIB_PATH)


def test_abi_version_is_still_2_with_verify_sample(B):
    assert re.search(r"^#define L2Z_ABI_VERSION 2$", open(B.HEADER_PATH).read(), flags=re.M)
    assert B.lib().l2z_abi_version() == 2
    assert NAME in B.declared_symbols("product")


def test_verify_header_no_longer_lists_sampled_speculation_as_out_of_scope(B):
    txt = open(B.HEADER_PATH).read()
    assert "OUT OF SCOPE: sampled speculation" not in txt
    assert "COIN INVARIANCE" in txt


def test_binding_has_verify_sample_speculate_sample_and_coin_stream(B):
    for name in ("verify_sample", "verify_sample_time", "verify_logits"):
        assert callable(getattr(B.RunState, name, None)), name
    assert callable(getattr(B, "speculate_sample", None))
    assert callable(getattr(B, "coin_stream", None))
    assert len(B.lib().l2z_verify_sample.argtypes) == 11
    assert len(B.lib().l2z_verify_sample_time.argtypes) == 11


def test_coin_stream_is_the_cli_generators_stream(B):
    H = C.CDLL(os.path.join(HOST, "libllama2_host.so"))
    H.l2zh_prng_floats.argtypes = [C.c_uint64, C.POINTER(C.c_float), C.c_size_t]
    H.l2zh_prng_floats.restype = None
    for seed, n in ((0, 1), (1, 7), (42, 300), (2 ** 63 + 5, 33)):
        want = (C.c_float * n)()
        H.l2zh_prng_floats(seed, want, n)
        got = B.coin_stream(seed, n)
        assert got.dtype == np.float32 and got.shape == (n,)
        assert np.array_equal(got.view(np.uint32), np.array(want[:], np.float32).view(np.uint32)), seed
        assert np.all((got >= 0.0) & (got < 1.0))
    assert B.coin_stream(3, 0).size == 0
    # a prefix of a longer stream: coin g is a function of (seed, g)
    assert np.array_equal(B.coin_stream(9, 5), B.coin_stream(9, 50)[:5])
    assert not np.array_equal(B.coin_stream(9, 5), B.coin_stream(10, 5))


def test_speculate_sample_refuses_bad_k_and_too_few_coins_before_any_device_call(B):
    class S:   # (never reaches a call)
        cfg = B.L2ZConfig(8, 16, 1, 2, 2, 10, 12)
    with pytest.raises(ValueError):
        B.speculate_sample(S(), None, [3, 4], 0, 16, 1.0, 0.9, np.zeros(64, np.float32))
    with pytest.raises(ValueError):
        B.speculate_sample(S(), None, [3, 4], 0, -1, 1.0, 0.9, np.zeros(64, np.float32))
    with pytest.raises(ValueError):   # 12 positions, 2 of them the prompt's: 10 coins
        B.speculate_sample(S(), None, [3, 4], 0, 4, 1.0, 0.9, np.zeros(9, np.float32))
    with pytest.raises(ValueError):
        B.speculate_sample(S(), None, [3, 4], 8, 4, 1.0, 0.9, np.zeros(5, np.float32))


class _FakeState:
    """speculate_sample's view of a runstate, the model replaced by a hash: the token after a history is a function of that
    history and the coin it is drawn with -- what COIN INVARIANCE assumes of the device"""

    def __init__(self, B, seq_len, log):
        self.cfg, self.seen, self.log = B.L2ZConfig(8, 16, 1, 2, 2, 50, seq_len), [], log

    @staticmethod
    def draw(history, coin):
        h = hash((tuple(int(t) for t in history), float(np.float32(coin)))) & 0xFFFFFF
        return 2 + h % 48   # never BOS

    def prefill(self, tokens, pos0, w):
        assert pos0 == 0
        self.seen = [int(t) for t in tokens]

    def sample_first(self, coin):
        self.log.append((len(self.seen) - 1, float(coin)))
        return self.draw(self.seen, coin)

    def verify_sample(self, tokens, pos0, w, temperature, top_p, coins):
        assert len(coins) == len(tokens) and pos0 == len(self.seen)   # one coin per row; the call starts at the next position
        hist, nxt = list(self.seen), []
        for i, t in enumerate(tokens):
            hist.append(int(t))
            self.log.append((pos0 + i, float(coins[i])))
            nxt.append(self.draw(hist, coins[i]))
        a = 0
        while a + 1 < len(tokens) and int(tokens[a + 1]) == nxt[a]:
            a += 1
        self.seen += [int(t) for t in tokens[:a + 1]]
        return np.array(nxt, np.int32), a


def test_speculate_sample_hands_coins_out_per_position(B, monkeypatch):
    """The loop alone, the model mocked: every position is drawn with ITS coin in every call that draws it, whatever the
    drafter and K, so the ids are the K = 0 ids."""
    monkeypatch.setattr(B, "sample_batch", lambda states, t, p, c: np.array([states[0].sample_first(c)], np.int32))
    steps, prompt = 40, [5, 6, 7]
    coins = B.coin_stream(12, steps - len(prompt))
    log = []
    base, st0 = B.speculate_sample(_FakeState(B, 64, log), None, prompt, steps, 0, 1.0, 0.9, coins)
    assert len(base) == steps and base[:3].tolist() == prompt and st0["offered"] == 0
    # position p (the row that reads the token at p) draws generated token p - len(prompt) with that coin
    assert log == [(len(prompt) + g, float(coins[g])) for g in range(steps - len(prompt))]
    full = np.concatenate([[1], base]).astype(np.int32)
    rng = np.random.default_rng(3)

    def half_wrong(hist, k):
        g = full[len(hist):len(hist) + k].copy()
        bad = rng.random(len(g)) < 0.5
        g[bad] = (g[bad] - 2 + 1) % 48 + 2
        return g

    for k in (1, 4, 15):
        for drafter in (lambda h, kk: full[len(h):len(h) + kk], half_wrong, lambda h, kk: full[len(h):len(h) + kk] * 0 + 2,
                        lambda h, kk: full[len(h):len(h) + max(0, kk - 2)], None):
            log = []
            toks, stats = B.speculate_sample(_FakeState(B, 64, log), None, prompt, steps, k, 1.0, 0.9, coins, drafter)
            assert toks.tolist() == base.tolist(), k
            for pos, coin in log:   # a rejected row's position is drawn again with the same coin
                assert coin == float(coins[pos - len(prompt)]), (k, pos)
            assert stats["emitted"] == steps - len(prompt) - 1 and stats["accepted"] <= stats["offered"]
    # the last call before seq_len is shorter: no row beyond the last position
    log = []
    toks, _ = B.speculate_sample(_FakeState(B, 40, log), None, prompt, 0, 15, 1.0, 0.9, coins, lambda h, kk: full[len(h):len(h) + kk])
    assert toks.tolist() == base.tolist() and max(p for p, _ in log) == 39


def test_cli_lists_spec_sample_and_refuses_what_does_not_combine(B):
    r = subprocess.run([EXE, "-h"], capture_output=True, text=True)
    assert "--spec-sample" in r.stdout
    # (a.bin does not exist: a run that got as far as the checkpoint would say so instead)
    cases = [(["--spec-sample", "4", "--spec", "4"], "with --spec:"),
             (["--spec", "4", "--spec-sample", "4", "-t", "0"], "with --spec:"),
             (["--spec-sample", "4", "-b", "2"], "--batch"),
             (["--spec-sample", "4", "-g", "2"], "--gpus"),
             (["--spec-sample", "4", "--score"], "--score"),
             (["--spec-sample", "4", "-t", "0", "-b", "2"], "--batch"),
             (["--spec-sample", "16"], "0 to 15"),
             (["--spec-sample", "-1"], "0 to 15"),
             (["--spec-sample", "x"], "0 to 15"),
             (["--spec-sample", "4", "-t", "-0.5"], "temperature")]
    for args, what in cases:
        r = subprocess.run([EXE, "a.bin", *args], capture_output=True, text=True)
        assert r.returncode != 0, args
        assert "--spec-sample" in r.stderr and what in r.stderr, (args, r.stderr)
        assert "cannot open checkpoint" not in r.stderr, args
    for args in (["--spec-sample", "4"], ["--spec-sample", "0", "-t", "0.8", "-p", "1"], ["--spec-sample", "15", "-t", "0"]):
        r = subprocess.run([EXE, "a.bin", *args], capture_output=True, text=True)
        assert r.returncode != 0 and "cannot open checkpoint" in r.stderr, args   # accepted: got as far as the file


def test_cli_spec_keeps_its_refusal_at_a_temperature(B):
    r = subprocess.run([EXE, "a.bin", "--spec", "4"], capture_output=True, text=True)
    assert r.returncode != 0 and "--spec" in r.stderr and "-t 0" in r.stderr
    assert "cannot open checkpoint" not in r.stderr


_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
B = ge.load_package().binding
L = B.lib()
tok = (C.c_int32 * 2)(1, 2)
out = (C.c_int32 * 2)(0, 0)
coins = (C.c_float * 2)(0.25, 0.5)
acc = C.c_int(0)
cfg = B.L2ZConfig(8, 16, 1, 2, 2, 10, 4)
print(L.l2z_verify_sample(tok, 2, 0, 1.0, 0.9, coins, C.byref(cfg), None, None, out, C.byref(acc)))
"""


def test_verify_sample_without_a_device_returns_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    assert out.split() == [str(B.ERR_NO_DEVICE)], out
