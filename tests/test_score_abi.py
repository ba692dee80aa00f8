"""l2z_score without a GPU: the symbol is declared in the product header, listed in the version script, exported by both
libraries and bound in the Zig shim with the header's nine parameters; the ABI version stays 2; the slab hook stays out of
the product library; the binding has RunState.score; the CLI lists --score and refuses it with -b / -g before any device
is touched."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "llama2.zig_amd", "host")
EXE = os.path.join(HOST, "llama2")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines()}


def test_score_is_declared_mapped_exported_and_bound(B):
    assert "l2z_score" in B.declared_symbols("product")
    mp = open(os.path.join(ROOT, "llama2.zig_amd", "csrc", "llama2_hip.map")).read()
    assert "l2z_score" in set(re.findall(r"^\s+(l2z_\w+);", mp, flags=re.M))
    assert "l2z_score" in exported(B.PRODUCT_LIB_PATH)
    assert "l2z_score" in exported(B.LIB_PATH)
    z = open(os.path.join(ROOT, "bindings", "zig", "llama2_hip.zig")).read()
    hdr = re.sub(r"/\*.*?\*/", "", open(B.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"pub extern fn l2z_score\(([^)]*)\)", z, flags=re.S)
    assert m, "llama2_hip.zig does not declare l2z_score"
    h = re.search(r"\bl2z_score\s*\(([^)]*)\)", hdr, flags=re.S)
    n_zig = len([a for a in m.group(1).split(",") if a.strip()])
    n_hdr = len([a for a in h.group(1).split(",") if a.strip()])
    assert n_zig == n_hdr == 9


def test_abi_version_is_still_2(B):
    assert re.search(r"^#define L2Z_ABI_VERSION 2$", open(B.HEADER_PATH).read(), flags=re.M)
    assert B.lib().l2z_abi_version() == 2


def test_slab_hook_is_test_only(B):
    assert "l2z_score_slab_set" in B.declared_symbols("test")
    assert "l2z_score_slab_set" not in B.declared_symbols("product")
    assert "l2z_score_slab_set" not in exported(B.PRODUCT_LIB_PATH)
    assert "l2z_score_slab_set" in exported(B.LIB_PATH)


def test_binding_has_score(B):
    assert callable(getattr(B.RunState, "score", None))
    assert callable(getattr(B.RunState, "score_slab_set", None))
    assert B.lib().l2z_score.argtypes is not None and len(B.lib().l2z_score.argtypes) == 9


def test_cli_lists_score_and_refuses_it_with_batch_or_gpus(B):
    r = subprocess.run([EXE, "-h"], capture_output=True, text=True)
    assert "--score" in r.stdout
    # (a.bin does not exist: a run that got as far as the checkpoint would say so instead)
    r = subprocess.run([EXE, "a.bin", "--score", "-b", "2"], capture_output=True, text=True)
    assert r.returncode != 0 and "--score does not combine with --batch" in r.stderr
    r = subprocess.run([EXE, "a.bin", "--score", "-g", "2"], capture_output=True, text=True)
    assert r.returncode != 0 and "--score does not combine with --gpus" in r.stderr
