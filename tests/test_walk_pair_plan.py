"""walk_pair_plan.h — whether the last range of a launch is walked in pairs (kernels_walk_pair.hip; tuning knobs walk_pair,
walk_pair_cache): tests/cxx/walk_pair_plan_check.cpp runs the flagship's launch and every condition of the pair kernel's domain
through the header on a CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")


def test_the_pair_walk_follows_its_rule(tmp_path):
    exe = tmp_path / "walk_pair_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "walk_pair_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK 32 cases")
