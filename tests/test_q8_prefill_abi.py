"""The batched prompt pass on int8 group-quantized weights and what stands around it, without a GPU (after
tests/test_q8_abi.py): l2z_prefill_q8 and its two hooks are PREVIEW entry points -- declared in the test header only,
absent from the version script and from the product library, exported by the test library, bound in the Python binding
with matching argument lists; the product header still declares its 31 functions and ABI version 2; without a device the
calls fail with L2Z_ERR_NO_DEVICE, or L2Z_ERR_INVALID where the arguments themselves are wrong."""
import ctypes as C
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = {"l2z_prefill_q8": 6, "l2z_q8_quantize_rows": 7, "l2z_q8_gemm": 9}


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


def test_the_three_names_are_declared_in_the_test_header_only(B):
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


def test_the_three_names_are_exported_by_the_test_library_only(B):
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    in_map = set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    product, test = exported(B.PRODUCT_LIB_PATH), exported(B.LIB_PATH)
    assert len(in_map) == 31
    for name in NAMES:
        assert name not in in_map
        assert name not in product
        assert name in test
    assert not any(s.startswith("l2z") and "q8" in s for s in product)


def test_the_binding_s_argument_lists_match_the_header(B):
    i32p, i8p, fp, vp = C.POINTER(C.c_int32), C.POINTER(C.c_int8), C.POINTER(C.c_float), C.c_void_p
    cfgp = C.POINTER(B.L2ZConfig)
    want = {"l2z_prefill_q8": [i32p, C.c_int, C.c_int, cfgp, vp, vp],
            "l2z_q8_quantize_rows": [fp, C.c_int, C.c_size_t, fp, C.c_int, i8p, fp],
            "l2z_q8_gemm": [fp, i8p, fp, C.c_int, i8p, fp, C.c_size_t, C.c_size_t, C.c_int]}
    for name, types in want.items():
        at = getattr(B.lib(), name).argtypes
        assert at is not None and list(at) == types, name
        assert len(types) == NAMES[name]
    assert callable(B.RunState.prefill_q8) and callable(B.q8_quantize_rows) and callable(B.q8_gemm) and callable(B.generate_q8)


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
i8p, fp, i32p = C.POINTER(C.c_int8), C.POINTER(C.c_float), C.POINTER(C.c_int32)
toks = np.array([3, 4], np.int32)
print(L.l2z_prefill_q8(toks.ctypes.data_as(i32p), 2, 0, C.byref(cfg), None, None))
x = np.ones((2, 32), np.float32)
q = np.zeros((2, 32), np.int8)
s = np.zeros((2, 1), np.float32)
print(L.l2z_q8_quantize_rows(x.ctypes.data_as(fp), 2, 32, None, 32, q.ctypes.data_as(i8p), s.ctypes.data_as(fp)))
wq = np.zeros((4, 32), np.int8)
ws = np.zeros((4, 1), np.float32)
out = np.zeros((2, 4), np.float32)
print(L.l2z_q8_gemm(out.ctypes.data_as(fp), q.ctypes.data_as(i8p), s.ctypes.data_as(fp), 2, wq.ctypes.data_as(i8p),
                    ws.ctypes.data_as(fp), 32, 4, 32))
# what is wrong with the arguments themselves is said without a device too
print(L.l2z_q8_quantize_rows(x.ctypes.data_as(fp), 2, 32, None, 48, q.ctypes.data_as(i8p), s.ctypes.data_as(fp)))
print(L.l2z_q8_quantize_rows(x.ctypes.data_as(fp), 0, 32, None, 32, q.ctypes.data_as(i8p), s.ctypes.data_as(fp)))
print(L.l2z_q8_gemm(out.ctypes.data_as(fp), q.ctypes.data_as(i8p), s.ctypes.data_as(fp), 2, wq.ctypes.data_as(i8p),
                    ws.ctypes.data_as(fp), 32, 3, 32))
print(L.l2z_q8_gemm(None, q.ctypes.data_as(i8p), s.ctypes.data_as(fp), 2, wq.ctypes.data_as(i8p), ws.ctypes.data_as(fp), 32, 4, 32))
"""


def test_calls_without_a_device_return_no_device_or_invalid(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    nd, inv = str(B.ERR_NO_DEVICE), str(B.ERR_INVALID)
    assert out.split() == [nd, nd, nd, inv, inv, inv, inv], out
