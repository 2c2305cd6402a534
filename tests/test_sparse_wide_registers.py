"""Register budget of the wide learned-sparse kernels (kernels_sparse.hip: pools of 64 * R keys per wave, R = 2, 4, 8, 16), read from
the built object like tests/test_kernel_registers.py reads the narrow ones.  A block is 256 threads around a 32 KB accumulator
tile, so LDS allows four waves per SIMD; 128 VGPRs is four waves per SIMD from the 512-register file: up to there registers are
not the binding limit.  Nothing may go to scratch memory: a pool indexed through memory is the slow way to keep it."""
import pytest

from tests.test_kernel_registers import _find, _kernels


@pytest.mark.parametrize("R", [2, 4, 8, 16])
def test_wide_sparse_kernels_keep_four_waves_per_simd_and_no_scratch(tmp_path, R):
    ks = _kernels("kernels_sparse.o", tmp_path)
    for name in (f"sparse_tile_kernel<{R}>",            # unpacked layout (R = 1 is the narrow kernel)
                 f"sparse_wide_packed_kernel<{R}>",     # packed layout
                 f"sparse_wide_finish_kernel<{R}>"):
        k = _find(ks, name)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_count"] <= 128, (name, k)

