"""The layout of a llama2.c version-2 checkpoint body (llama2.zig_amd/csrc/q8_layout.h: every tensor's byte offset and size,
the total, the refusals -- a bad group size, dimensions that do not divide, a body that is too short) without a GPU:
tests/q8_layout_check.cpp, a stand-alone program with its own main over that header alone, built with
-fsanitize=address,undefined and run.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = ["totals of the named shapes", "the pieces cover the body once, in the file's order", "refusals", "tensor names"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("q8_layout") / "q8_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "llama2.zig_amd", "csrc"),
                    os.path.join(HERE, "q8_layout_check.cpp"), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    return run.returncode, run.stdout + run.stderr


def test_the_program_ran_clean_under_the_sanitizers(report):
    code, out = report
    assert code == 0, out
    assert "ERROR" not in out and "runtime error" not in out and "FAILED" not in out, out


@pytest.mark.parametrize("case", CASES)
def test_case(report, case):
    assert f"ok: {case}" in report[1].splitlines(), report[1]
