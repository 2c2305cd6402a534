"""Device check of three wave primitives the walks rest on: group_reduce_add_u32 at every group size, vis_alias_winners ("the lower slot
wins" when two neighbours alias one filter bit) and div_rn_unscaled (the bits of the IEEE quotient, on the operands the walk can form and
on the range device_common.h states), against plain host models (tests/cxx/topk_check_host.h; its CPU self-test is run by
test_gpu_topk_select.py).  Integers and bit patterns: exact."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _compile(out, extra=()):
    src = os.path.join(ROOT, "tests", "cxx", "wave_prims_check.hip")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "cosdata_amd", "csrc"),
                           *extra, src, "-o", str(out)])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_wave_prims_check_compiles_for_gfx950(tmp_path):
    _compile(tmp_path / "wave_prims_check.o", extra=("-c",))


@pytest.mark.gpu
def test_wave_prims_match_host_models(tmp_path):
    exe = tmp_path / "wave_prims_check"
    _compile(exe)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout
