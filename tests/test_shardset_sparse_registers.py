"""Register and LDS budget of the kernels behind the learned-sparse search on a shard set (kernels_sparse.hip: the record form of the two
finish kernels, sparse_fold_rerank_kernel<N>), read from the built object like tests/test_sparse_wide_registers.py reads the wide
ones.  Nothing may go to scratch memory, and the fold keeps exactly its N keys in LDS."""
import os
import re
import subprocess

import pytest

from tests.test_kernel_registers import LLVM, _find, _kernels

FOLD_WIDTHS = [256, 512, 1024, 2048, 4096, 8192]


def _lds_bytes(tmp_path):
    """group_segment_fixed_size per kernel, from the code object _kernels() has extracted into tmp_path"""
    dev = [f for f in os.listdir(tmp_path) if "amdgcn" in f and "gfx950" in f]
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", dev[0]], cwd=str(tmp_path), check=True, capture_output=True, text=True).stdout
    out, size = {}, None
    for line in notes.splitlines():                       # (.group_segment_fixed_size comes before .name inside a kernel's entry)
        m = re.match(r"\s+(?:- )?\.group_segment_fixed_size:\s+(\d+)", line)
        if m:
            size = int(m.group(1))
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m and size is not None:
            out[subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()] = size
            size = None
    return out


@pytest.fixture(scope="module")
def sparse_object(tmp_path_factory):
    d = tmp_path_factory.mktemp("sparse_obj")
    ks = _kernels("kernels_sparse.o", d)
    return ks, _lds_bytes(d)


def test_record_kernels_use_no_scratch(sparse_object):
    ks, lds = sparse_object
    k = _find(ks, "sparse_record_kernel(")
    assert k["private_segment_fixed_size"] == 0, k
    for R in (2, 4, 8, 16):
        name = f"sparse_wide_record_kernel<{R}>"
        k = _find(ks, name)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)
        # best[64 R] u64 + the candidate count: what sparse_wide_finish_kernel<R> holds
        assert _find(lds, name) <= 64 * R * 8 + 16, (name, _find(lds, name))


@pytest.mark.parametrize("N", FOLD_WIDTHS)
def test_fold_kernel_keeps_n_keys_in_lds_and_no_scratch(sparse_object, N):
    ks, lds = sparse_object
    name = f"sparse_fold_rerank_kernel<{N}u>"
    k = _find(ks, name)
    assert k["private_segment_fixed_size"] == 0, (name, k)
    assert k["vgpr_count"] <= 128, (name, k)
    # buf[N] u64 and nothing else — the gathered keys, then the compact list of re-ranked candidates and its fill count in the same
    # words: N * 8 bytes, 64 KB at N = 8192
    assert _find(lds, name) == N * 8, (name, _find(lds, name))
