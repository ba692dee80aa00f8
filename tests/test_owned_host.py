"""The scratch owner and the grow rule (llama2.zig_amd/csrc/owned.h: a move-only owner of one allocation, and the one
all-or-nothing rule by which a group of them grows) without a GPU: tests/owned_check.cpp, a stand-alone program with its own
main over that header alone, which supplies the two raw functions over malloc with a live set and a failing N-th allocation,
built with -fsanitize=address,undefined and run.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = ["move leaves the source null and frees once", "reset twice is harmless",
         "grow at the same capacity and key allocates nothing",
         "grow to a larger need drains, frees each old member once and records the rounded capacity",
         "a changed key at an equal capacity remakes the group",
         "a failed allocation leaves the group empty, and the next grow succeeds",
         "destroying an owner struct with a half-built group leaves the live set empty"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("owned") / "owned_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "llama2.zig_amd", "csrc"),
                    os.path.join(HERE, "owned_check.cpp"), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    return run.returncode, run.stdout + run.stderr


def test_the_program_ran_clean_under_the_sanitizers(report):
    code, out = report
    assert code == 0, out
    assert "ERROR" not in out and "runtime error" not in out, out


@pytest.mark.parametrize("case", CASES)
def test_case(report, case):
    assert f"ok: {case}" in report[1].splitlines(), report[1]
