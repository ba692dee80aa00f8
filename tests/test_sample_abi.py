"""The on-device sampler and the prompt fork without a GPU: l2z_sample_batch / l2z_runstate_fork are declared, exported by
the product library, listed in its version script and bound in the Zig shim with the header's arity; the test hook
l2z_logits_write stays out of the product library; without a device both calls fail with L2Z_ERR_NO_DEVICE; the host
library draws the CLI's numbers and samples with a given number; the CLI lists -b."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "llama2.zig_amd", "host")
SYMS = ("l2z_sample_batch", "l2z_runstate_fork")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


def test_sample_symbols_are_declared_exported_mapped_and_bound(B):
    assert set(SYMS) <= set(B.declared_symbols("product"))
    assert set(SYMS) <= exported(B.PRODUCT_LIB_PATH)
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    assert set(SYMS) <= set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    z = open(os.path.join(ROOT, "bindings", "zig", "llama2_hip.zig")).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(B.HEADER_PATH).read(), flags=re.S)
    for s in SYMS:
        m = re.search(rf"pub extern fn {s}\(([^)]*)\)", z, flags=re.S)
        assert m, s
        h = re.search(rf"\b{s}\s*\(([^)]*)\)", hdr, flags=re.S)
        n_zig = len([a for a in m.group(1).split(",") if a.strip()])
        n_hdr = len([a for a in h.group(1).split(",") if a.strip()])
        assert n_zig == n_hdr == {"l2z_sample_batch": 6, "l2z_runstate_fork": 3}[s]


def test_logits_hook_is_test_only(B):
    assert "l2z_logits_write" in B.declared_symbols("test")
    assert "l2z_logits_write" not in B.declared_symbols("product")
    assert "l2z_logits_write" not in exported(B.PRODUCT_LIB_PATH)
    assert "l2z_logits_write" in exported(B.LIB_PATH)


_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
B = ge.load_package().binding
L = B.lib()
ss = (C.c_void_p * 1)(None)
f = (C.c_float * 1)(0.5)
out = (C.c_int32 * 1)(0)
print(L.l2z_sample_batch(1, ss, f, f, f, out), L.l2z_runstate_fork(None, None, 0))
"""


def test_sample_calls_without_a_device_return_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    assert out.split() == [str(B.ERR_NO_DEVICE)] * 2, out


def host_lib():
    L = C.CDLL(os.path.join(HOST, "libllama2_host.so"))
    fp = C.POINTER(C.c_float)
    L.l2zh_prng_open.restype = C.c_void_p
    L.l2zh_prng_open.argtypes = [C.c_uint64]
    L.l2zh_prng_close.argtypes = [C.c_void_p]
    L.l2zh_prng_next_f32.restype = C.c_float
    L.l2zh_prng_next_f32.argtypes = [C.c_void_p]
    L.l2zh_prng_floats.argtypes = [C.c_uint64, fp, C.c_size_t]
    L.l2zh_sample_rng.restype = C.c_size_t
    L.l2zh_sample_rng.argtypes = [fp, C.c_size_t, C.c_void_p]
    L.l2zh_sample_top_p_rng.restype = C.c_size_t
    L.l2zh_sample_top_p_rng.argtypes = [fp, C.c_size_t, C.c_float, C.c_void_p, fp]
    L.l2zh_sample_coin.restype = C.c_size_t
    L.l2zh_sample_coin.argtypes = [fp, C.c_size_t, C.c_float]
    L.l2zh_sample_top_p_coin.restype = C.c_size_t
    L.l2zh_sample_top_p_coin.argtypes = [fp, C.c_size_t, C.c_float, C.c_float, fp]
    return L


def test_host_coin_entry_points_replay_the_generator(B):
    """l2zh_prng_next_f32 is the stream l2zh_prng_floats gives for the seed, and sampling with the drawn number is the
    sampler that draws it itself (both samplers, ties and near-uniform distributions over 32000 tokens)."""
    H = host_lib()
    rng = H.l2zh_prng_open(77)
    got = np.array([H.l2zh_prng_next_f32(rng) for _ in range(64)], np.float32)
    H.l2zh_prng_close(rng)
    want = (C.c_float * 64)()
    H.l2zh_prng_floats(77, want, 64)
    assert np.array_equal(got, np.array(want[:], np.float32))
    g = np.random.default_rng(3)
    for V in (4, 1000, 32000):
        w = np.round(g.uniform(1.0, 2.0, V) * 16) / 16
        p = (w / w.sum()).astype(np.float32)
        pp = p.ctypes.data_as(C.POINTER(C.c_float))
        for top_p in (0.0, 0.5, 0.9, 1.0):
            a, b = H.l2zh_prng_open(V), H.l2zh_prng_open(V)
            for _ in range(8):
                coin = H.l2zh_prng_next_f32(b)
                if top_p in (0.0, 1.0):
                    assert H.l2zh_sample_rng(pp, V, a) == H.l2zh_sample_coin(pp, V, coin)
                else:
                    assert H.l2zh_sample_top_p_rng(pp, V, top_p, a, None) == H.l2zh_sample_top_p_coin(pp, V, top_p, coin, None)
            H.l2zh_prng_close(a)
            H.l2zh_prng_close(b)


def test_cli_usage_lists_batch_and_checks_it(B):
    exe = os.path.join(HOST, "llama2")
    r = subprocess.run([exe, "-h"], capture_output=True, text=True)
    assert "-b, --batch <int>" in r.stdout
    for bad in ("0", "17", "x"):
        r = subprocess.run([exe, "a.bin", "-b", bad], capture_output=True, text=True)
        assert r.returncode == 1 and "unable to use --batch" in r.stderr
    r = subprocess.run([exe, "a.bin", "-b", "2", "-g", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "shard groups are not batched" in r.stderr
