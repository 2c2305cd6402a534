"""Binary / octal codes and f16 / f32 rows in the latency kernels: the domain rule, the kernel the plan picks, the f16 tile's row
stride and the LDS of both kernels are plain integer logic in walk_plan.h — tests/cxx/walk_lat_storages_check.cpp runs them on a CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")


def test_latency_storages_plan_and_lds(tmp_path):
    exe = tmp_path / "walk_lat_storages_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "cxx", "walk_lat_storages_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK "), out.stdout + out.stderr
