"""Learned-sparse search on a shard set, without a device: the numpy model of the exact scheme (per-shard candidate records + fold,
tests/shardset_sparse_world.py) against the oracle over the whole collection, the host-only plan of the fold
(cosdata_amd/csrc/sparse_fold_plan.h), and the three entry points in the header and the built library."""
import ctypes as C
import os
import re
import subprocess

import pytest

from tests import shardset_sparse_world as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["cos_shardset_attach_sparse", "cos_shardset_sparse_search_batch", "cos_shardset_hybrid_search_mixed"]

# (bounds, bits, thr, top_k, factor): every configuration the scheme was argued on
MODEL_CASES = ([(W.BOUNDS3, b, t, 10, 5) for b, t in W.CONFIGS] + [(W.BOUNDS8, 6, 0.0, 12, 5), (W.BOUNDS8, 4, 0.5, 50, 5)] +
               [(W.BOUNDS3, b, t, k, 0) for b, t in W.CONFIGS for k in (10, 64)])


@pytest.mark.parametrize("bounds,bits,thr,top_k,factor", MODEL_CASES)
def test_record_and_fold_model_is_the_whole_collections_answer(bounds, bits, thr, top_k, factor):
    w = W.world(bits)
    assert w.differing(w.model, bounds, thr, top_k, factor) == 0


def test_per_shard_rerank_and_merge_is_not(capsys):
    """the scheme the set does NOT use differs on most queries with a rerank, on none without one — and the corpus exercises the
    two-key order at the cut"""
    W.assert_preconditions()
    w = W.world(6)
    assert w.differing(w.wrong_scheme, W.BOUNDS8, 0.0, 12, 5) >= 20
    assert w.differing(w.wrong_scheme, W.BOUNDS3, 0.0, 10, 0) == 0
    w4 = W.world(4)
    _, _, short = W.cut_statistics(w4, W.BOUNDS8, 0.5, 250)
    assert short >= 1, "the (bits 4, thr 0.5, C 250) case is there for the queries with fewer than C candidates"


def _plan_program(tmp_path):
    src = tmp_path / "plan.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "sparse_fold_plan.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "    namespace p = sparse_fold_plan;\n"
                   "    const unsigned S = atoi(argv[1]), B = atoi(argv[3]); const unsigned long long C = atoll(argv[2]); const int rr = atoi(argv[4]);\n"
                   "    const p::Plan pl = p::plan(S, C); const p::Layout l = p::layout(B, C, rr != 0);\n"
                   '    printf("%u %d %llu %u %u %zu %zu %zu\\n", pl.N, pl.status, (unsigned long long)pl.keys, pl.lds_bytes(), l.stride, l.counts, l.raw, l.words);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "plan"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "cosdata_amd", "csrc"), str(src), "-o", str(exe)])
    return lambda S, Cn, B=1, rr=1: tuple(map(int, subprocess.check_output([str(exe), str(S), str(Cn), str(B), str(rr)]).split()))


def test_plan_picks_the_fold_width_and_refuses_above_8192(tmp_path):
    plan = _plan_program(tmp_path)
    OK, INVALID, UNIMPLEMENTED = 0, 3, 4
    # (S, C) -> (N, status, gathered keys): the stride is C rounded up to 64 .. 1024, N the power of two >= S * stride, at least 256
    for S, Cn, N, keys in [(1, 1, 256, 64), (3, 50, 256, 192), (3, 60, 256, 192), (3, 65, 512, 384), (8, 12, 512, 512), (8, 250, 2048, 2048),
                           (8, 1024, 8192, 8192), (8, 1000, 8192, 8192), (5, 600, 8192, 5120), (1, 1024, 1024, 1024), (2, 512, 1024, 1024),
                           (128, 64, 8192, 8192)]:
        got = plan(S, Cn)
        assert got[:4] == (N, OK, keys, N * 8), (S, Cn, got)
    for S, Cn in [(9, 1024), (9, 513), (129, 1), (17, 512)]:
        got = plan(S, Cn)
        assert got[:2] == (0, UNIMPLEMENTED) and got[2] > 8192, (S, Cn, got)
    assert plan(3, 1025)[:2] == (0, UNIMPLEMENTED)
    assert plan(0, 10)[:2] == (0, INVALID) and plan(3, 0)[:2] == (0, INVALID)
    # the record: keys u64 [B][stride] | counts [B] padded to an even word count | raw u32 [B][stride] when the call reranks
    assert plan(3, 50, B=40, rr=1)[4:] == (64, 2 * 40 * 64, 2 * 40 * 64 + 40, 3 * 40 * 64 + 40)
    assert plan(3, 50, B=41, rr=1)[4:] == (64, 2 * 41 * 64, 2 * 41 * 64 + 42, 3 * 41 * 64 + 42)
    assert plan(3, 250, B=7, rr=0)[4:] == (256, 2 * 7 * 256, 2 * 7 * 256 + 8, 2 * 7 * 256 + 8)
    for B in (1, 2, 5, 256):                               # S records side by side keep their u64 keys aligned
        for rr in (0, 1):
            assert plan(2, 100, B=B, rr=rr)[7] % 2 == 0


def test_header_declares_and_library_exports_the_three_entry_points():
    from cosdata_amd import _lib
    header = open(os.path.join(ROOT, "include", "cosdata_hip.h")).read()
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", header), name
        assert hasattr(L, name), name
        assert name in _lib.ABI_SYMBOLS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int32 and fn.argtypes, name
    assert len(L.cos_shardset_attach_sparse.argtypes) == 4
    assert len(L.cos_shardset_sparse_search_batch.argtypes) == 11
    assert len(L.cos_shardset_hybrid_search_mixed.argtypes) == 5


def test_null_and_zero_arguments_are_invalid_without_a_device():
    from cosdata_amd import _lib
    L = _lib.lib()
    INVALID = 3
    one = (C.c_uint32 * 4)()
    f = (C.c_float * 4)()
    p = lambda a: C.cast(a, C.c_void_p)
    fake = C.c_void_p(8)                                   # a non-null set is never reached: another argument refuses the call first
    assert L.cos_shardset_attach_sparse(None, None, 0, None) == INVALID
    assert L.cos_shardset_sparse_search_batch(None, p(one), p(f), p(one), 1, 1, 0.0, 0, p(one), p(f), p(one)) == INVALID
    assert L.cos_shardset_sparse_search_batch(fake, None, p(f), p(one), 1, 1, 0.0, 0, p(one), p(f), p(one)) == INVALID
    assert L.cos_shardset_sparse_search_batch(fake, p(one), p(f), p(one), 0, 1, 0.0, 0, p(one), p(f), p(one)) == INVALID
    assert L.cos_shardset_sparse_search_batch(fake, p(one), p(f), p(one), 1, 0, 0.0, 0, p(one), p(f), p(one)) == INVALID
    assert L.cos_shardset_sparse_search_batch(fake, p(one), p(f), p(one), 1, 1, 0.0, 0, None, p(f), p(one)) == INVALID
    rq = _lib.CosHybridRequest()
    rq.struct_size = C.sizeof(_lib.CosHybridRequest)
    assert L.cos_shardset_hybrid_search_mixed(None, C.byref(rq), p(one), p(f), p(one)) == INVALID
    assert L.cos_shardset_hybrid_search_mixed(fake, None, p(one), p(f), p(one)) == INVALID
    assert L.cos_shardset_hybrid_search_mixed(fake, C.byref(rq), p(one), p(f), p(one)) == INVALID      # B == 0, top_k == 0
    rq.B, rq.top_k = 1, 1
    assert L.cos_shardset_hybrid_search_mixed(fake, C.byref(rq), p(one), p(f), p(one)) == INVALID      # arm == NULL
    rq.struct_size = 8
    assert L.cos_shardset_hybrid_search_mixed(fake, C.byref(rq), p(one), p(f), p(one)) == INVALID
    assert "struct_size" in L.cos_last_error_string().decode()
