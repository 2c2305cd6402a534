"""Device check of the shared exact-rerank header (cosdata_amd/csrc/exact_rerank.h): a miniature rerank built only from the header and
dot_engines.h — pair and oct dot, the pair passes, the LDS form, write_topk in both forms — against a host model of the reference's
rule written in tests/cxx/exact_rerank_check.hip (eight fused chains, their pairwise tree, an unfused tail, the negative NaN of 0/0,
the larger id first on ties).  Everything compared is a u64 key or the bits of an output word: exact."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")
HIPCC = "/opt/rocm/bin/hipcc"


def _compile(out, extra=()):
    # the library's floating-point flags: the rule is written with explicit fma / mul / add and an IEEE division
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
                           "-I", os.path.join(ROOT, "cosdata_amd", "csrc"), *extra, os.path.join(CXX, "exact_rerank_check.hip"), "-o", str(out)])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_exact_rerank_check_compiles_for_gfx950(tmp_path):
    _compile(tmp_path / "exact_rerank_check.o", extra=("-c",))


@pytest.mark.gpu
def test_exact_rerank_matches_host_model(tmp_path):
    exe = tmp_path / "exact_rerank_check"
    _compile(exe)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout
