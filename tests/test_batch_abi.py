"""The batched decode step's C ABI without a GPU: l2z_transformer_batch / l2z_argmax_batch are declared, exported by the
product library, listed in its version script and bound in the Zig shim; L2Z_BATCH_MAX is 16; without a device both
fail with L2Z_ERR_NO_DEVICE."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "llama2_hip.h")
SYMS = ("l2z_transformer_batch", "l2z_argmax_batch")


def test_batch_symbols_are_declared_exported_mapped_and_bound(B):
    assert set(SYMS) <= set(B.declared_symbols("product"))
    out = subprocess.run(["nm", "-D", "--defined-only", B.PRODUCT_LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines()}
    assert set(SYMS) <= exported
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    assert set(SYMS) <= set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    z = open(os.path.join(ROOT, "bindings", "zig", "llama2_hip.zig")).read()
    for s in SYMS:
        assert f"pub extern fn {s}(" in z


def test_batch_max_is_16(B):
    txt = open(HEADER).read()
    assert re.search(r"^#define L2Z_BATCH_MAX 16\b", txt, flags=re.M)
    assert B.BATCH_MAX == 16
    assert re.search(r"#define L2Z_ABI_VERSION 2\b", txt)


_CHILD = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
B = ge.load_package().binding
L = B.lib()
tok = (C.c_int32 * 1)(1)
pos = (C.c_int32 * 1)(0)
ss = (C.c_void_p * 1)(None)
out = (C.c_int32 * 1)(0)
cfg = B.L2ZConfig(8, 16, 1, 2, 2, 10, 4)
print(L.l2z_transformer_batch(1, tok, pos, C.byref(cfg), ss, None), L.l2z_argmax_batch(1, ss, out))
"""


def test_batch_calls_without_a_device_return_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env,
                         timeout=120).stdout
    assert out.split() == [str(B.ERR_NO_DEVICE)] * 2, out
