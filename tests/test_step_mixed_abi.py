"""l2z_step_mixed and what stands around it, without a GPU: a PREVIEW entry point -- declared in the test header only, with
its eleven parameters and L2Z_MIXED_ROWS_MAX 512, absent from the version script and from the product library, exported by
the test library, bound in the Python binding (binding.step_mixed, binding.serve, binding.MIXED_ROWS_MAX); the product
header still declares its 31 functions and ABI version 2; without a device the call fails with L2Z_ERR_NO_DEVICE."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "l2z_step_mixed"


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


def test_step_mixed_is_declared_in_the_test_header_only(B):
    assert NAME in B.declared_symbols("test")
    assert NAME not in B.declared_symbols("product")
    hdr = re.sub(r"/\*.*?\*/", "", open(B.TEST_HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bl2z_step_mixed\s*\(([^)]*)\)", hdr, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 11
    assert re.search(r"^#define L2Z_MIXED_ROWS_MAX 512$", open(B.TEST_HEADER_PATH).read(), flags=re.M)
    assert NAME not in open(B.HEADER_PATH).read()
    # ... and the product header is what it was: 31 functions at ABI version 2
    assert len(B.declared_symbols("product")) == 31
    assert re.search(r"^#define L2Z_ABI_VERSION 2$", open(B.HEADER_PATH).read(), flags=re.M)
    assert B.lib().l2z_abi_version() == 2


def test_step_mixed_is_exported_by_the_test_library_only(B):
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    assert NAME not in set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    assert NAME not in exported(B.PRODUCT_LIB_PATH)
    assert NAME in exported(B.LIB_PATH)
    assert not any(s.startswith("l2z") and "step_mixed" in s for s in exported(B.PRODUCT_LIB_PATH))


def test_binding_has_step_mixed_and_serve(B):
    assert callable(getattr(B, "step_mixed", None))
    assert callable(getattr(B, "serve", None))
    assert B.MIXED_ROWS_MAX == 512
    at = B.lib().l2z_step_mixed.argtypes
    assert at is not None and len(at) == 11


_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
B = ge.load_package().binding
L = B.lib()
tok = (C.c_int32 * 3)(1, 2, 3)
nt = (C.c_int32 * 2)(1, 2)
p0 = (C.c_int32 * 2)(0, 0)
ss = (C.c_void_p * 2)(None, None)
nxt = (C.c_int32 * 2)(0, 0)
cfg = B.L2ZConfig(8, 16, 1, 2, 2, 10, 4)
print(L.l2z_step_mixed(2, tok, nt, p0, None, None, None, C.byref(cfg), ss, None, nxt))
"""


def test_step_mixed_without_a_device_returns_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    assert out.split() == [str(B.ERR_NO_DEVICE)], out
