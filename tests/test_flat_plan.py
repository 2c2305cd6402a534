"""The host-only part of the exhaustive scans (cosdata_amd/csrc/flat_plan.h) is plain integer logic: the limits, the pool widths, the
chunk schedule of an attempt, the buffer sizes that follow from it and the kernel that scores a fused chunk.
tests/golden/flat_plan_cases.txt holds the expected chunk lists and values, written by hand; tests/cxx/flat_plan_check.cpp reads them and
is a program of its own, built with the address and undefined-behaviour sanitizers, so a wrapped product or a schedule that does not
end fails it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")


def test_header_stands_alone():
    """plain C++17: no HIP header, no handle, nothing of the library"""
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-x", "c++", "-"],
                         input='#include "flat_plan.h"\n', capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_schedules_and_limits_under_sanitizers(tmp_path):
    exe = tmp_path / "flat_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "flat_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "flat_plan_cases.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip() == "OK"
