"""Device check of the shared top-k header (cosdata_amd/csrc/topk_select.h), primitive by primitive: bitonic_sort_desc, bitonic_merge_desc,
merge_sorted_desc, Pool<R> (scripts of insert_at / pop_head / rank_of / peek* / pool_fold_*), fold_stream and the LDS networks, at every
width the kernels instantiate, against plain host models (tests/cxx/topk_check_host.h).  Everything compared is a u64 key: exact.
The self-test runs on a CPU and proves that the verifiers reject damaged output and that no case leaves the header's contract."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")
HIPCC = "/opt/rocm/bin/hipcc"


def _compile(out, extra=()):
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "cosdata_amd", "csrc"),
                           *extra, os.path.join(CXX, "topk_select_check.hip"), "-o", str(out)])


def test_verifiers_reject_damaged_output_and_cases_keep_the_contract(tmp_path):
    exe = tmp_path / "topk_check_selftest"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(CXX, "topk_check_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1].startswith("OK"), r.stdout


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_topk_select_check_compiles_for_gfx950(tmp_path):
    _compile(tmp_path / "topk_select_check.o", extra=("-c",))


@pytest.mark.gpu
def test_topk_select_matches_host_models(tmp_path):
    exe = tmp_path / "topk_select_check"
    _compile(exe)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("OK"), r.stdout
