"""The layout of an l2z_step_mixed call (llama2.zig_amd/csrc/mixed_plan.h: rows -> sequences and positions, the decode list,
the prompt rows, the flash tile list, the last rows, the deepest decode position) without a GPU: tests/mixed_plan_check.cpp,
a stand-alone program with its own main over that header alone, built with -fsanitize=address,undefined and run.  Every row
is named exactly once, the classes are disjoint and complete, tiles never cross a sequence, and the lists stay in bounds at
n = 128, R = 512 and at n = 1, R = 1.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = ["one sequence of one row", "128 sequences, 512 rows", "a mix of the classes",
         "the deepest one-row sequence sizes the decode grid", "tiles are ordered by key rows, ties in sequence order", "refusals"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("mixed_plan") / "mixed_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "llama2.zig_amd", "csrc"),
                    os.path.join(HERE, "mixed_plan_check.cpp"), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    return run.returncode, run.stdout + run.stderr


def test_the_program_ran_clean_under_the_sanitizers(report):
    code, out = report
    assert code == 0, out
    assert "ERROR" not in out and "runtime error" not in out, out


@pytest.mark.parametrize("case", CASES)
def test_case(report, case):
    assert f"ok: {case}" in report[1].splitlines(), report[1]
