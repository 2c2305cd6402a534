"""The launch policy of a dense search (cosdata_amd/csrc/walk_plan.h) is plain integer logic: checked here without a GPU.
tests/golden/walk_plan_cases.txt records, for a grid of inputs on both sides of every threshold, what the commit before the header
decided in its four places (scripts/gen_walk_plan_cases.cpp, built against that commit); tests/cxx/walk_plan_check.cpp replays every
line through the header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")
CASES = os.path.join(ROOT, "tests", "golden", "walk_plan_cases.txt")


def test_header_stands_alone():
    """plain C++17: no HIP header, no handle, nothing of the library"""
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-x", "c++", "-"],
                         input='#include "walk_plan.h"\n', capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_every_recorded_decision_is_reproduced(tmp_path):
    exe = tmp_path / "walk_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "walk_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), CASES], capture_output=True, text=True)
    n_cases = sum(1 for line in open(CASES) if line.strip() and not line.startswith("#"))
    assert n_cases >= 500
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-3000:]
    assert out.stdout.split()[:3] == ["OK", str(n_cases), "cases,"] and out.stdout.split()[3] == "0"   # no line skipped, none differing
