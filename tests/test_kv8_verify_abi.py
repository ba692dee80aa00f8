"""l2z_verify_kv8 and what stands around it, without a GPU: three PREVIEW names -- declared in the test header
only, present in the loaded test library and bound in the Python binding; the product header still declares its 31
functions; without a device the call fails with L2Z_ERR_NO_DEVICE."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["l2z_verify_kv8", "l2z_verify_kv8_time", "l2z_kv8_verify_attention"]


def test_the_names_are_declared_in_the_test_header_only_and_exported(B):
    assert len(B.declared_symbols("product")) == 31
    for name in NAMES:
        assert name in B.declared_symbols("test") and name not in B.declared_symbols("product")
        assert hasattr(B.lib(), name) and getattr(B.lib(), name).argtypes is not None
    assert all(callable(getattr(B.RunState, m, None)) for m in ("verify_kv8", "verify_kv8_time"))
    assert callable(getattr(B, "kv8_verify_attention", None))


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
B = ge.load_package().binding
s = B.RunState.__new__(B.RunState)
s.cfg, s.h = B.L2ZConfig(8, 16, 1, 2, 2, 12, 4), None
try:
    s.verify_kv8([1, 2, 3], 0, s)
except B.L2ZError as e:
    print(e.code)
"""


def test_verify_kv8_without_a_device_raises_no_device(B):
    """A process that sees no device (on a GPU machine too: the child hides them all)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _CHILD, ROOT], check=True, capture_output=True, text=True, env=env, timeout=120).stdout
    assert out.split() == [str(B.ERR_NO_DEVICE)], out
