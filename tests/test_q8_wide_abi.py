"""The wide step on int8 group-quantized weights and its GEMM form, without a GPU (after tests/test_q8_batch_abi.py): PREVIEW
entry points -- declared in the test header only, absent from the version script and from the product library, exported by
the test library, bound with matching argument lists; without a device the calls fail with L2Z_ERR_NO_DEVICE."""
import ctypes as C
import os
import re
import subprocess
import sys

from test_q8_batch_abi import ROOT, exported

NAMES = {"l2z_transformer_wide_q8": 7, "l2z_q8_gemm_wide": 9, "l2z_q8_gemm_epi": 11}


def test_the_names_are_declared_and_exported_by_the_test_side_only(B):
    hdr = re.sub(r"/\*.*?\*/", "", open(B.TEST_HEADER_PATH).read(), flags=re.S)
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    product, test = exported(B.PRODUCT_LIB_PATH), exported(B.LIB_PATH)
    for name, n_params in NAMES.items():
        assert name in B.declared_symbols("test") and name not in B.declared_symbols("product")
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n_params, name
        assert name not in open(B.HEADER_PATH).read() and name not in mp
        assert name not in product and name in test
    assert len(B.declared_symbols("product")) == 31 and B.lib().l2z_abi_version() == 2


def test_the_binding_s_argument_lists_match_the_header(B):
    i32p, fp, i8p, vp, sz = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_int8), C.c_void_p, C.c_size_t
    want = {"l2z_transformer_wide_q8": [C.c_int, i32p, i32p, C.POINTER(B.L2ZConfig), C.POINTER(vp), vp, i32p],
            "l2z_q8_gemm_wide": [fp, i8p, fp, C.c_int, i8p, fp, sz, sz, C.c_int],
            "l2z_q8_gemm_epi": [C.c_int, C.c_int, fp, i8p, fp, C.c_int, i8p, fp, sz, sz, C.c_int]}
    for name, types in want.items():
        assert list(getattr(B.lib(), name).argtypes) == types and len(types) == NAMES[name], name
    assert all(callable(f) for f in (B.transformer_wide_q8, B.generate_wide_q8, B.q8_gemm_wide, B.q8_gemm_epi))


_CHILD = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg = ge.load_package()
B, ck = pkg.binding, pkg.checkpoint
cfg = B.L2ZConfig(*[int(v) for v in ck.Config(64, 192, 1, 4, 2, 64, 8).as_i32()])
i32p = C.POINTER(C.c_int32)
toks, pos, nxt = np.array([3, 4], np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
states = (C.c_void_p * 2)()
print(B.lib().l2z_transformer_wide_q8(2, toks.ctypes.data_as(i32p), pos.ctypes.data_as(i32p), C.byref(cfg), states, None,
                                      nxt.ctypes.data_as(i32p)))
try:
    B.q8_gemm_wide(np.ones((17, 64), np.int8), np.ones((17, 1), np.float32), np.ones((4, 64), np.int8), np.ones((4, 1), np.float32), 64)
except B.L2ZError as e:
    print(e.code)
"""


def test_calls_without_a_device_return_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env, timeout=120).stdout
    assert out.split() == [str(B.ERR_NO_DEVICE)] * 2, out
