"""The host-only part of the mixed hybrid call (cosdata_amd/csrc/hybrid_plan.h) is plain integer logic: the split of arm[] into the
dense / sparse / BM25 sub-batches and the refusals decided before anything is enqueued.  tests/cxx/hybrid_plan_check.cpp holds the
expected positions and statuses, written by hand; it is a program of its own, built with the address and undefined-behaviour
sanitizers, so a slot written past the batch or a wrapped width fails it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")


def test_header_stands_alone():
    """plain C++17: no HIP header, no handle, nothing of the library"""
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-x", "c++", "-"],
                         input='#include "hybrid_plan.h"\n', capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_split_and_refusals_under_sanitizers(tmp_path):
    exe = tmp_path / "hybrid_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "hybrid_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip() == "OK"
