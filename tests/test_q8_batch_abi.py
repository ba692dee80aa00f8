"""The batched step and the verify pass on int8 group-quantized weights and their two timing twins, without a GPU (after
tests/test_q8_prefill_abi.py): PREVIEW entry points -- declared in the test header only, absent from the version script and
from the product library, exported by the test library, bound in the Python binding with matching argument lists; the
product header still declares its 31 functions and ABI version 2, and the product library exports what its version script
lists; without a device the calls fail with L2Z_ERR_NO_DEVICE, or L2Z_ERR_INVALID where the arguments themselves are
wrong."""
import ctypes as C
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = {"l2z_transformer_batch_q8": 6, "l2z_verify_q8": 11, "l2z_batch_q8_time": 8, "l2z_verify_q8_time": 11}


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


def test_the_names_are_declared_in_the_test_header_only(B):
    hdr = re.sub(r"/\*.*?\*/", "", open(B.TEST_HEADER_PATH).read(), flags=re.S)
    product = open(B.HEADER_PATH).read()
    for name, n_params in NAMES.items():
        assert name in B.declared_symbols("test")
        assert name not in B.declared_symbols("product")
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n_params, name
        assert name not in product
    assert "q8" not in product
    assert len(B.declared_symbols("product")) == 31
    assert re.search(r"^#define L2Z_ABI_VERSION 2$", product, flags=re.M)
    assert B.lib().l2z_abi_version() == 2


def test_the_names_are_exported_by_the_test_library_only(B):
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    in_map = set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    product, test = exported(B.PRODUCT_LIB_PATH), exported(B.LIB_PATH)
    assert len(in_map) == 31
    for name in NAMES:
        assert name not in in_map
        assert name not in product
        assert name in test
    # the product library's export list is unchanged: the version script's names, which are the product header's
    assert {s for s in product if s.startswith("l2z")} == in_map == set(B.declared_symbols("product"))
    assert not any(s.startswith("l2z") and "q8" in s for s in product)


def test_the_binding_s_argument_lists_match_the_header(B):
    i32p, fp, vp, ip = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p, C.POINTER(C.c_int)
    cfgp, dp = C.POINTER(B.L2ZConfig), C.POINTER(C.c_double)
    want = {"l2z_transformer_batch_q8": [C.c_int, i32p, i32p, cfgp, C.POINTER(vp), vp],
            "l2z_verify_q8": [i32p, C.c_int, C.c_int, C.c_float, C.c_float, fp, cfgp, vp, vp, i32p, ip],
            "l2z_batch_q8_time": [C.c_int, i32p, i32p, cfgp, C.POINTER(vp), vp, C.c_int, dp],
            "l2z_verify_q8_time": [i32p, C.c_int, C.c_int, C.c_float, C.c_float, fp, cfgp, vp, vp, C.c_int, dp]}
    for name, types in want.items():
        at = getattr(B.lib(), name).argtypes
        assert at is not None and list(at) == types, name
        assert len(types) == NAMES[name]
    for f in (B.transformer_batch_q8, B.batch_q8_time, B.RunState.verify_q8, B.RunState.verify_q8_time, B.speculate_q8):
        assert callable(f)


_CHILD = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package()
B, ck = pkg.binding, pkg.checkpoint
L = B.lib()
c = ck.Config(64, 192, 1, 4, 2, 64, 8)
cfg = B.L2ZConfig(*[int(v) for v in c.as_i32()])
i32p = C.POINTER(C.c_int32)
toks = np.array([3, 4], np.int32)
pos = np.array([0, 0], np.int32)
nxt = np.zeros(2, np.int32)
acc = C.c_int(0)
ms = C.c_double(0.0)
states = (C.c_void_p * 2)()
tp, pp, np_ = toks.ctypes.data_as(i32p), pos.ctypes.data_as(i32p), nxt.ctypes.data_as(i32p)
print(L.l2z_transformer_batch_q8(2, tp, pp, C.byref(cfg), states, None))
print(L.l2z_verify_q8(tp, 2, 0, C.c_float(0.0), C.c_float(1.0), None, C.byref(cfg), None, None, np_, C.byref(acc)))
print(L.l2z_batch_q8_time(2, tp, pp, C.byref(cfg), states, None, 1, C.byref(ms)))
print(L.l2z_verify_q8_time(tp, 2, 0, C.c_float(0.0), C.c_float(1.0), None, C.byref(cfg), None, None, 1, C.byref(ms)))
# what is wrong with the arguments themselves is said without a device too
print(L.l2z_batch_q8_time(2, tp, pp, C.byref(cfg), states, None, 0, C.byref(ms)))
print(L.l2z_verify_q8_time(tp, 2, 0, C.c_float(0.0), C.c_float(1.0), None, C.byref(cfg), None, None, 0, C.byref(ms)))
"""


def test_calls_without_a_device_return_no_device_or_invalid(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    nd, inv = str(B.ERR_NO_DEVICE), str(B.ERR_INVALID)
    assert out.split() == [nd, nd, nd, nd, inv, inv], out
