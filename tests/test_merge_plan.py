"""The host-only part of the S-way merge (cosdata_amd/csrc/merge_plan.h) is plain integer logic: which kernel sorts the S * k keys of a
query, how wide it is, and when the call is refused.  tests/cxx/merge_plan_check.cpp is a program of its own, built with the address and
undefined-behaviour sanitizers: every boundary (1024 / 1025, 2048 / 2049, 4096 / 4097, 8192 / 8193), S = 1, k = 1 and products of S and
k that do not fit 32 bits."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")


def test_header_stands_alone():
    """plain C++17: no HIP header, no handle, nothing of the library"""
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-x", "c++", "-"],
                         input='#include "merge_plan.h"\n', capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_widths_and_refusals_under_sanitizers(tmp_path):
    exe = tmp_path / "merge_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "merge_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip() == "OK"


def test_the_launch_code_reads_the_plan():
    """kernels_misc.hip decides nothing of its own: both families of entry points go through merge_plan::plan"""
    src = open(os.path.join(CSRC, "kernels_misc.hip")).read()
    assert '#include "merge_plan.h"' in src and "merge_plan::plan(S, k, max_keys)" in src
    assert src.count("merge_plan::WAVE_MAX_KEYS") >= 2 and src.count("merge_plan::LDS_MAX_KEYS") >= 2
