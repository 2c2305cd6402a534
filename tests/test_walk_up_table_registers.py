"""Register budgets of the two walk kernels that carry the flagship launches, after the level under the table got its third copy of
the row-level rounds (walk_kernel.inc, `UPT`): read from the built object like tests/test_kernel_registers.py.  The variant is one
more instruction stream inside the same kernel, so the kernel's register count is the largest of its streams: it must stay on the
step of the VGPR ladder the kernel was on, with nothing in scratch.

                                          commit before   ladder step
  walk_kernel<0, 1, 2, true, false, 8>    75 VGPRs        80 = 6 waves per SIMD   (12.5M x 1024 shard, ef 112)
  walk_kernel<0, 1, 1, true, false, 8>    71 VGPRs        72 = 7 waves per SIMD   (1M x 768 corpus, ef 64)

A first form of the change — the neighbours' nodes one level up as a plain u32 array beside adj_mag, i.e. one more pointer alive
through the level's rounds — measured 77 and 71 + 12 bytes of scratch here; with the norm and the node in one array behind one
pointer (LevelDev::adj_up) both kernels keep the counts of the commit before."""
from tests.test_kernel_registers import _find, _kernels


def test_flagship_walk_kernels_stay_on_their_ladder_step(tmp_path):
    ks = _kernels("kernels_walk.o", tmp_path)
    r2 = _find(ks, "walk_kernel<0, 1, 2, true, false, 8>")
    r1 = _find(ks, "walk_kernel<0, 1, 1, true, false, 8>")
    print("walk_kernel<0, 1, 2, true, false, 8>", r2, "walk_kernel<0, 1, 1, true, false, 8>", r1)
    assert r2["private_segment_fixed_size"] == 0 and r1["private_segment_fixed_size"] == 0
    assert r2["vgpr_count"] <= 80      # the commit before: 75
    assert r1["vgpr_count"] <= 72      # the commit before: 71
