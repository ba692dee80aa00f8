"""l2z_verify_wide and what stands around it, without a GPU: a PREVIEW entry point -- declared in the test header only, with
twelve parameters, absent from the version script and from the product library, exported by the test library, bound in
the Python binding (binding.verify_wide and the loop binding.speculate_wide); the product header still declares its 31
functions and ABI version 2; without a device the call fails with L2Z_ERR_NO_DEVICE."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "l2z_verify_wide"


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


def test_verify_wide_is_declared_in_the_test_header_only_with_twelve_parameters(B):
    assert NAME in B.declared_symbols("test")
    assert NAME not in B.declared_symbols("product")
    hdr = re.sub(r"/\*.*?\*/", "", open(B.TEST_HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bl2z_verify_wide\s*\(([^)]*)\)", hdr, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 12


def test_verify_wide_is_exported_by_the_test_library_only(B):
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    assert NAME not in set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    assert NAME not in exported(B.PRODUCT_LIB_PATH)
    assert NAME in exported(B.LIB_PATH)
    assert not any(s.startswith("l2z") and "wide" in s for s in exported(B.PRODUCT_LIB_PATH))


def test_the_loops_share_one_text_and_the_batch_loop_keeps_its_limits(B):
    """speculate_batch still refuses a 17th sequence; speculate_wide takes up to 128 and refuses a 129th (no device needed:
    the refusals come before anything touches one)"""
    with pytest.raises(ValueError):
        B.speculate_batch([None] * 17, None, [[1]] * 17, 4, 3)
    with pytest.raises(ValueError):
        B.speculate_wide([None] * 129, None, [[1]] * 129, 4, 3)
    with pytest.raises(ValueError):
        B.speculate_wide([None] * 2, None, [[1]] * 2, 4, 16)


def test_product_header_still_declares_31_functions_at_abi_version_2(B):
    assert len(B.declared_symbols("product")) == 31
    assert re.search(r"^#define L2Z_ABI_VERSION 2$", open(B.HEADER_PATH).read(), flags=re.M)
    assert B.lib().l2z_abi_version() == 2


def test_binding_has_verify_wide_and_speculate_wide(B):
    assert callable(getattr(B, "verify_wide", None))
    assert callable(getattr(B, "speculate_wide", None))
    at = B.lib().l2z_verify_wide.argtypes
    assert at is not None and len(at) == 12


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
nxt = (C.c_int32 * 3)()
acc = (C.c_int32 * 2)()
cfg = B.L2ZConfig(8, 16, 1, 2, 2, 10, 4)
print(L.l2z_verify_wide(2, tok, nt, p0, None, None, None, C.byref(cfg), ss, None, nxt, acc))
"""


def test_verify_wide_without_a_device_returns_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    assert out.split() == [str(B.ERR_NO_DEVICE)], out
