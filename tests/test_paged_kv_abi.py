"""The paged KV cache's surface without a GPU: six PREVIEW entry points -- declared in the test header only, absent from the
version script and from the product library, exported by the test library, bound in the Python binding with the header's
parameter counts (binding.KvPool, RunState(cfg, pool=...), RunState.pages / trim); L2Z_KV_PAGE is 64; the product header
still declares its 31 functions and ABI version 2; without a device l2z_kvpool_init fails with L2Z_ERR_NO_DEVICE."""
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# name -> parameters in include/llama2_hip_test.h
NAMES = {"l2z_kvpool_init": 3, "l2z_kvpool_free": 1, "l2z_kvpool_info": 4, "l2z_runstate_init_paged": 3,
         "l2z_runstate_pages": 4, "l2z_runstate_trim": 2}


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_in_the_test_header_only_with_its_parameters(B, name):
    assert name in B.declared_symbols("test")
    assert name not in B.declared_symbols("product")
    hdr = re.sub(r"/\*.*?\*/", "", open(B.TEST_HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == NAMES[name]


def test_page_size_is_64(B):
    assert re.search(r"^#define L2Z_KV_PAGE 64\b", open(B.TEST_HEADER_PATH).read(), flags=re.M)
    assert B.KV_PAGE == 64


def test_exported_by_the_test_library_only(B):
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    in_map = set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    prod, test = exported(B.PRODUCT_LIB_PATH), exported(B.LIB_PATH)
    for name in NAMES:
        assert name not in in_map, name
        assert name not in prod, name
        assert name in test, name
    assert not any(s.startswith("l2z") and ("kvpool" in s or "paged" in s) for s in prod)


def test_product_header_still_declares_31_functions_at_abi_version_2(B):
    assert len(B.declared_symbols("product")) == 31
    assert re.search(r"^#define L2Z_ABI_VERSION 2$", open(B.HEADER_PATH).read(), flags=re.M)
    assert B.lib().l2z_abi_version() == 2


def test_binding_has_the_pool_and_the_paged_runstate(B):
    import inspect
    assert inspect.isclass(getattr(B, "KvPool", None))
    assert callable(getattr(B.KvPool, "info", None)) and callable(getattr(B.KvPool, "close", None))
    assert "pool" in inspect.signature(B.RunState.__init__).parameters
    assert callable(getattr(B.RunState, "pages", None)) and callable(getattr(B.RunState, "trim", None))
    for name, n in NAMES.items():
        at = getattr(B.lib(), name).argtypes
        assert at is not None and len(at) == n, name


_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
B = ge.load_package().binding
L = B.lib()
cfg = B.L2ZConfig(8, 16, 1, 2, 2, 10, 4)
pool = C.c_void_p()
print(L.l2z_kvpool_init(C.byref(cfg), 4, C.byref(pool)), pool.value)
"""


def test_kvpool_init_without_a_device_returns_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    assert out.split() == [str(B.ERR_NO_DEVICE), "None"], out
