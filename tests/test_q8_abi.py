"""The int8 group-quantized entry points and what stands around them, without a GPU: PREVIEW entry points -- declared in
the test header only, absent from the version script and from the product library, exported by the test library, bound in
the Python binding; the product header still declares its 31 functions and ABI version 2; without a device the calls fail
with L2Z_ERR_NO_DEVICE."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = {"l2z_weights_init_q8": 7, "l2z_weights_init_q8_from": 3, "l2z_weights_q8_read": 5, "l2z_q8_quantize": 5,
         "l2z_q8_matmul": 8, "l2z_q8_matvec_case": 1}


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


def test_q8_entry_points_are_declared_in_the_test_header_only(B):
    hdr = re.sub(r"/\*.*?\*/", "", open(B.TEST_HEADER_PATH).read(), flags=re.S)
    product = open(B.HEADER_PATH).read()
    for name, n_params in NAMES.items():
        assert name in B.declared_symbols("test")
        assert name not in B.declared_symbols("product")
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n_params, name
        assert name not in product
    assert "q8" not in product
    # ... and the product header is what it was: 31 functions at ABI version 2
    assert len(B.declared_symbols("product")) == 31
    assert re.search(r"^#define L2Z_ABI_VERSION 2$", product, flags=re.M)
    assert B.lib().l2z_abi_version() == 2


def test_q8_entry_points_are_exported_by_the_test_library_only(B):
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    in_map = set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    product, test = exported(B.PRODUCT_LIB_PATH), exported(B.LIB_PATH)
    for name in NAMES:
        assert name not in in_map
        assert name not in product
        assert name in test
    assert not any(s.startswith("l2z") and "q8" in s for s in product)


def test_binding_has_the_q8_wrappers(B, ck):
    for name, n_params in NAMES.items():
        at = getattr(B.lib(), name).argtypes
        assert at is not None and len(at) == n_params, name
    assert callable(B.Weights.from_q8) and callable(B.Weights.quantized) and callable(B.Weights.q8_read)
    assert callable(B.q8_quantize) and callable(B.q8_matmul) and callable(B.q8_matvec_case)
    for fn in ("quantize_q80", "v2_layout", "write_checkpoint_v2", "read_checkpoint_v2"):
        assert callable(getattr(ck, fn))


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
body = np.zeros(ck.v2_layout(c, True, 32).total, np.uint8)
h = C.c_void_p()
i8p, fp = C.POINTER(C.c_int8), C.POINTER(C.c_float)
print(L.l2z_weights_init_q8(C.byref(cfg), body.ctypes.data_as(C.c_void_p), body.size, 1, 32, None, C.byref(h)))
x = np.ones(32, np.float32)
q = np.zeros(32, np.int8)
s = np.zeros(1, np.float32)
print(L.l2z_q8_quantize(x.ctypes.data_as(fp), 32, 32, q.ctypes.data_as(i8p), s.ctypes.data_as(fp)))
out = np.zeros(1, np.float32)
print(L.l2z_q8_matmul(out.ctypes.data_as(fp), q.ctypes.data_as(i8p), s.ctypes.data_as(fp), q.ctypes.data_as(i8p),
                      s.ctypes.data_as(fp), 32, 1, 32))
# what is wrong with the arguments themselves is said without a device too
print(L.l2z_weights_init_q8(C.byref(cfg), body.ctypes.data_as(C.c_void_p), body.size, 1, 48, None, C.byref(h)))
print(L.l2z_weights_init_q8(C.byref(cfg), body.ctypes.data_as(C.c_void_p), body.size - 1, 1, 32, None, C.byref(h)))
print(L.l2z_weights_init_q8_from(None, 32, C.byref(h)))
print(L.l2z_weights_q8_read(None, b"wq", 0, q.ctypes.data_as(i8p), s.ctypes.data_as(fp)))
case = B.Q8Case(epi=0, gs=32, n=32, rows0=1, q0=q.ctypes.data_as(i8p), s0=s.ctypes.data_as(fp), xq=q.ctypes.data_as(i8p),
                xs=s.ctypes.data_as(fp), out0=out.ctypes.data_as(fp), out0_len=1)
print(L.l2z_q8_matvec_case(C.byref(case)))
case.gs = 48
print(L.l2z_q8_matvec_case(C.byref(case)))
"""


def test_q8_calls_without_a_device_return_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    nd, inv = str(B.ERR_NO_DEVICE), str(B.ERR_INVALID)
    assert out.split() == [nd, nd, nd, inv, inv, inv, inv, nd, inv], out
