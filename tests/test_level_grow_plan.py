"""The host-only part of growing a graph's levels in front of a tail (cosdata_amd/csrc/level_grow_plan.h; the tail is the root on the base
graph, the pseudo nodes on the pseudo-root component) is plain integer logic: where a level's tail starts, how many nodes a level gains,
the node index and child link of every new node, and the renumbering of an old index.
tests/golden/level_grow_plan_cases.txt holds the expected values, written by hand; tests/cxx/level_grow_plan_check.cpp reads them and is a
program of its own, built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")


def test_header_stands_alone():
    """plain C++17: no HIP header, no handle, nothing of the library"""
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-x", "c++", "-"],
                         input='#include "level_grow_plan.h"\n', capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_growth_plans_under_sanitizers(tmp_path):
    """a level with no new node, every new node on level 0 only, a new node on the top level, Base replicas among the new rows, the
    pseudo root's child link after the level below grew; and the base graph's shapes: a tail of one node, a level that holds only the
    root, a level that gains nothing above one that gains, one new node that reaches the top level"""
    exe = tmp_path / "level_grow_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "level_grow_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "level_grow_plan_cases.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip() == "OK"
