"""The mixed hybrid call's entry points exist in the library, the ctypes table binds them with the header's struct layout, and
without a device the context is refused with NoDevice (the product path has no CPU fallback).  No compute here."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["cos_hybrid_create", "cos_hybrid_destroy", "cos_hybrid_search_mixed", "cos_sparse_search_batch_device"]


def test_library_exports_the_four_entry_points_and_the_table_binds_them():
    from cosdata_amd import _lib
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.ABI_SYMBOLS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int32 and fn.argtypes, name
    assert len(L.cos_hybrid_create.argtypes) == 2 and len(L.cos_hybrid_destroy.argtypes) == 1
    assert len(L.cos_hybrid_search_mixed.argtypes) == 8 and len(L.cos_sparse_search_batch_device.argtypes) == 12


def test_request_struct_layout_matches_header(tmp_path):
    from cosdata_amd._lib import CosHybridRequest
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cosdata_hip.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(cos_hybrid_request), offsetof(cos_hybrid_request, arm), '
                   'offsetof(cos_hybrid_request, bm25_offsets), offsetof(cos_hybrid_request, sparse_early_terminate_threshold), '
                   'offsetof(cos_hybrid_request, fusion_constant_k), COS_HYBRID_DENSE_SPARSE, COS_HYBRID_DENSE_BM25, COS_HYBRID_SPARSE_BM25);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sz, off_arm, off_bo, off_thr, off_k, a0, a1, a2 = map(int, subprocess.check_output([str(exe)]).split())
    assert C.sizeof(CosHybridRequest) == sz
    assert CosHybridRequest.arm.offset == off_arm and CosHybridRequest.bm25_offsets.offset == off_bo
    assert CosHybridRequest.sparse_early_terminate_threshold.offset == off_thr and CosHybridRequest.fusion_constant_k.offset == off_k
    import cosdata_amd as ca
    assert (ca.ARM_DENSE_SPARSE, ca.ARM_DENSE_BM25, ca.ARM_SPARSE_BM25) == (a0, a1, a2) == (0, 1, 2)


def test_context_without_a_device_is_no_device(gpu_available):
    """cos_hybrid_create: COS_ERR_NO_DEVICE (7) where no GPU is visible; where one is, the context opens and closes.  A NULL
    out pointer is Invalid (3) either way, and destroying NULL is a no-op."""
    import cosdata_amd as ca
    from cosdata_amd import _lib
    L = _lib.lib()
    assert L.cos_hybrid_create(0, None) == 3
    assert L.cos_hybrid_destroy(None) == 0
    h = C.c_void_p()
    rc = L.cos_hybrid_create(0, C.byref(h))
    if gpu_available:
        assert rc == 0 and h.value
        assert L.cos_hybrid_destroy(h) == 0
        with ca.HybridContext() as ctx:
            assert ctx._h.value
        assert not ctx._h.value
    else:
        assert rc == 7 and not h.value
        try:
            ca.HybridContext()
        except ca.CosdataError as e:
            assert e.status == 7
        else:
            raise AssertionError("HybridContext opened without a device")
    # the mixed call and the sparse device search refuse NULL handles before they touch a device
    assert L.cos_hybrid_search_mixed(None, None, None, None, None, None, None, None) == 3
    assert L.cos_sparse_search_batch_device(None, None, None, None, 1, 1, 0.0, 0, None, None, None, None) == 3
