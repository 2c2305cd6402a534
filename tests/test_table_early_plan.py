"""The two-part level-table GEMM is decided in cosdata_amd/csrc/walk_plan.h (WalkPlan::table_early_wgs): plain integer logic, checked here
without a GPU.  tests/golden/table_early_plan_cases.txt holds launches on both sides of every condition — not chained, tables under
2^30 entries, gated, knob above the item count, knob 0, the tile GEMM — with the expected values worked out by hand;
tests/cxx/table_early_plan_check.cpp replays every line through the header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")
CASES = os.path.join(ROOT, "tests", "golden", "table_early_plan_cases.txt")


def test_early_part_of_the_table_gemm_is_planned_as_recorded(tmp_path):
    exe = tmp_path / "table_early_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "table_early_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), CASES], capture_output=True, text=True)
    n_cases = sum(1 for line in open(CASES) if line.strip() and not line.startswith("#"))
    assert n_cases >= 20
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-3000:]
    assert out.stdout.split()[:3] == ["OK", str(n_cases), "cases,"] and out.stdout.split()[3] == "0"   # no line skipped, none differing
