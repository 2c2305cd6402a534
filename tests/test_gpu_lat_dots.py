"""Device check of the latency kernels' evaluation blocks (cosdata_amd/csrc/walk_common.h: stage_float_query, float_row_dot_wave,
spec_f32_dots, spec_f16_dots in both tile shapes, int_row_dot_group0 and spec_row_dots over binary / octal codes with 1 .. 4 chunk passes)
against the host models of tests/cxx/lat_dots_host.h, which tests/test_lat_dots_model.py pins to the oracle: every parked 64-bit word at
every candidate count T = 0 .. 256, at the dims on both sides of every tile, step and chunk-pass edge, under cosine and dot product, with
zero rows and a zero query among ordinary ones; every slot a block does not own keeps its sentinel.  Bit patterns: exact (a NaN: NaN on
both sides with the same sign)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosdata_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the library's flags for kernels_walk_lat.hip / kernels_walk_lat4.hip (csrc/Makefile)
PACKED_OFF = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt", *PACKED_OFF]


def _compile(out, extra=()):
    src = os.path.join(ROOT, "tests", "cxx", "lat_dots_check.hip")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", *FLAGS, "-I", CSRC, *extra, src, "-o", str(out)])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_lat_dots_check_compiles_for_gfx950_with_the_librarys_flags(tmp_path):
    _compile(tmp_path / "lat_dots_check.o", extra=("-c",))
    with open(os.path.join(CSRC, "Makefile")) as f:
        mk = f.read()
    # the two translation units the blocks ship in are still built without packed-f32 instructions, like this check
    rule = re.search(r"^kernels_walk_lat\.o kernels_walk_lat4\.o:\s*CXXFLAGS\s*\+=(.*)$", mk, re.M)
    assert rule and rule.group(1).split() == PACKED_OFF, "csrc/Makefile: the packed-f32 switch of kernels_walk_lat.o kernels_walk_lat4.o"
    base = re.search(r"^CXXFLAGS\s*:=(.*)$", mk, re.M).group(1).split()
    assert all(f in base for f in FLAGS[:4]), base


@pytest.mark.gpu
def test_lat_dots_match_host_models(tmp_path):
    exe = tmp_path / "lat_dots_check"
    _compile(exe)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout
