"""walk_plan.h's rule for the level that reads table columns for neighbours with a node one level up (WalkPlan::up_table_level,
tuning knob walk_up_table): tests/cxx/walk_up_table_plan_check.cpp replays tests/golden/walk_up_table_plan_cases.txt through the
header — expected values worked out by hand — and checks that knob 0, or no LevelDev::adj_up array, leave the plan as it was."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")


def test_up_table_level_follows_its_rule(tmp_path):
    exe = tmp_path / "walk_up_table_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "walk_up_table_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe), os.path.join(ROOT, "tests", "golden", "walk_up_table_plan_cases.txt")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK 17 cases")
