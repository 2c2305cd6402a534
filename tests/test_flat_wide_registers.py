"""Register budget of the exhaustive scans' selection / rerank kernels, read from the built objects like tests/test_kernel_registers.py
does.  The wide kernels (kernels_flat_wide.hip: pools of 64 * R keys per wave, R = 2, 4, 8, 16) keep their pool, one batch and the
sort's temporaries in registers: nothing may go to scratch memory, and 128 VGPRs (four waves per SIMD) is the ceiling.  The narrow
kernels (R = 1: top_k <= 12, k <= 32) are the ones the library had before wide pools existed and keep the registers they had there."""
import pytest

from tests.test_kernel_registers import _find, _kernels

# vgpr_count of the narrow kernels in kernels_flat.o built from commit 7f4bf1a (the parent of the wide pools)
NARROW_VGPRS = {
    "flat_select_segments(": 10,
    "flat_select_merge(": 12,
    "flat_select_append(": 12,
    "flat_rescore(": 56,
    "flat_rerank_top5k(": 66,
}


@pytest.mark.parametrize("R", [2, 4, 8, 16])
def test_wide_flat_kernels_use_no_scratch(tmp_path, R):
    ks = _kernels("kernels_flat_wide.o", tmp_path)
    for name in (f"flat_select_segments_w<{R}>", f"flat_select_merge_w<{R}>", f"flat_select_append_w<{R}>",
                 f"flat_rerank_w<{R}, false>", f"flat_rerank_w<{R}, true>"):
        k = _find(ks, name)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)


def test_narrow_flat_kernels_keep_the_registers_they_had(tmp_path):
    ks = _kernels("kernels_flat.o", tmp_path)
    for name, vgprs in NARROW_VGPRS.items():
        k = _find(ks, name)
        assert k["vgpr_count"] == vgprs and k["private_segment_fixed_size"] == 0, (name, k)
