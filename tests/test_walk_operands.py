"""CPU: the decisions behind the arrays a dense handle derives from its graph for the walk (cosdata_amd/csrc/walk_operands.h):
tests/cxx/walk_operands_check.cpp holds the level-table rule to the answers its measurements recorded (1M x 768 with neighbors_count 32,
a 12.5M x 1024 shard with 64; explicit max_cols, the 2^20 caps, a level without a node table, distinct keys) and to a restatement in
other words on random level sizes; the order-key level choice and its override's filter; the depth-first rank to a recursive walk on
random adjacency with empty slots, out-of-range entries and several components; and the operand state to what each GraphChange drops
and to one attempt per (graph, key)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")


def test_walk_operand_decisions(tmp_path):
    exe = tmp_path / "walk_operands_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "walk_operands_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
