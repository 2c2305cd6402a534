"""Register budgets of walk_kernel after its table levels got a second copy of their rounds for the nested level table
(walk_kernel.inc, `NEST`), read from the built object like tests/test_kernel_registers.py.  The variant is one more instruction stream
inside the same kernel, so a kernel's register count is the largest of its streams: no instantiation may take more VGPRs or more
scratch than it did at the commit before (tests/golden/walk_kernel_registers.txt), and the kernel that walks the flagship's table
levels — the upper range of the split walk, walk_kernel<0, 1, 2, true, false, 4> — keeps its 8 waves per SIMD (64 VGPRs)."""
import os
import re

from tests.test_kernel_registers import ROOT, _find, _kernels


def _recorded():
    out = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "walk_kernel_registers.txt")):
        if line.startswith("#"):
            continue
        counts, name = line.split("|")
        vgprs, scratch = (int(x) for x in counts.split())
        out[name.strip()] = (vgprs, scratch)
    return out


def test_no_walk_kernel_instantiation_grew(tmp_path):
    ks = _kernels("kernels_walk.o", tmp_path)
    built = {re.search(r"walk_kernel<[^>]*>", k).group(0): v for k, v in ks.items() if "walk_kernel<" in k}
    want = _recorded()
    assert set(built) == set(want)
    grown = {n: (want[n], (v["vgpr_count"], v["private_segment_fixed_size"])) for n, v in built.items()
             if v["vgpr_count"] > want[n][0] or v["private_segment_fixed_size"] > want[n][1]}
    print({n: (v["vgpr_count"], v["private_segment_fixed_size"]) for n, v in built.items() if (v["vgpr_count"], v["private_segment_fixed_size"]) != want[n]})
    assert not grown, grown


def test_the_table_levels_of_the_flagship_keep_eight_waves(tmp_path):
    ks = _kernels("kernels_walk.o", tmp_path)
    upper = _find(ks, "walk_kernel<0, 1, 2, true, false, 4>")
    lower = _find(ks, "walk_kernel<0, 1, 2, true, false, 8>")
    print("upper", upper, "lower", lower)
    assert upper["vgpr_count"] <= 64 and upper["private_segment_fixed_size"] == 0      # the commit before: 59
    assert lower["vgpr_count"] <= 80 and lower["private_segment_fixed_size"] == 0      # the commit before: 75
