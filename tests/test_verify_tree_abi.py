"""l2z_verify_tree and what stands around it, without a GPU: a PREVIEW entry point -- declared in the test header only, with
thirteen parameters, behind l2z_verify_batch, absent from the version script and from the product library, exported by the
test library, bound in the Python binding (RunState.verify_tree, speculate_tree, lookup_draft_tree); the product header
still declares its 31 functions and ABI version 2; without a device the call fails with L2Z_ERR_NO_DEVICE."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "l2z_verify_tree"


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


def test_verify_tree_is_declared_in_the_test_header_only(B):
    assert NAME in B.declared_symbols("test")
    assert NAME not in B.declared_symbols("product")
    assert "verify_tree" not in open(B.HEADER_PATH).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(B.TEST_HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bl2z_verify_tree\s*\(([^)]*)\)", hdr, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 13
    assert hdr.index("l2z_verify_batch") < m.start()   # in the preview section, behind the other preview entry points


def test_verify_tree_is_exported_by_the_test_library_only(B):
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    assert not any("verify_tree" in s for s in re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    assert not any(s.startswith("l2z") and "verify_tree" in s for s in exported(B.PRODUCT_LIB_PATH))
    assert {NAME, NAME + "_time"} <= exported(B.LIB_PATH)


def test_product_header_still_declares_31_functions_at_abi_version_2(B):
    assert len(B.declared_symbols("product")) == 31
    assert re.search(r"^#define L2Z_ABI_VERSION 2$", open(B.HEADER_PATH).read(), flags=re.M)
    assert B.lib().l2z_abi_version() == 2


def test_binding_has_verify_tree_speculate_tree_and_lookup_draft_tree(B):
    assert callable(getattr(B.RunState, "verify_tree", None))
    assert callable(getattr(B, "speculate_tree", None))
    assert callable(getattr(B, "lookup_draft_tree", None))
    at = B.lib().l2z_verify_tree.argtypes
    assert at is not None and len(at) == 13
    assert len(B.lib().l2z_verify_tree_time.argtypes) == 12


_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
B = ge.load_package().binding
L = B.lib()
tok = (C.c_int32 * 3)(1, 2, 3)
par = (C.c_int32 * 3)(-1, 0, 0)
nxt = (C.c_int32 * 3)()
path = (C.c_int32 * 3)()
acc = C.c_int(0)
cfg = B.L2ZConfig(8, 16, 1, 2, 2, 10, 4)
print(L.l2z_verify_tree(tok, par, 3, 0, C.c_float(0.0), C.c_float(1.0), None, C.byref(cfg), None, None, nxt, path, C.byref(acc)))
"""


def test_verify_tree_without_a_device_returns_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    assert out.split() == [str(B.ERR_NO_DEVICE)], out
