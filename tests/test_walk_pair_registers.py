"""Register budgets of walk_pair_kernel (kernels_walk_pair.hip: walk_kernel.inc compiled a second time with the pair code switched
on), read from the built object like tests/test_kernel_registers.py.  The kernel's resident waves are capped by LDS (a wave's layout
plus its dot cache: 14 waves per CU at the flagship's shape), so what matters is that no instantiation spills to scratch and that
none grows past the 96 VGPRs of five waves per SIMD; tests/golden/walk_pair_kernel_registers.txt records what they take.  walk_kernel's
own instantiations are held to their numbers by tests/test_walk_table_nested_registers.py, which this change leaves passing."""
import os
import re

from tests.test_kernel_registers import ROOT, _kernels


def _recorded():
    out = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "walk_pair_kernel_registers.txt")):
        if line.startswith("#"):
            continue
        counts, name = line.split("|")
        vgprs, scratch = (int(x) for x in counts.split())
        out[name.strip()] = (vgprs, scratch)
    return out


def test_pair_kernel_registers_and_scratch(tmp_path):
    ks = _kernels("kernels_walk_pair.o", tmp_path)
    built = {re.search(r"walk_pair_kernel<[^>]*>", k).group(0): (v["vgpr_count"], v["private_segment_fixed_size"]) for k, v in ks.items() if "walk_pair_kernel<" in k}
    want = _recorded()
    print(built)
    assert set(built) == set(want)
    for name, (vgprs, scratch) in built.items():
        assert scratch == 0 and vgprs <= 96, (name, vgprs, scratch)
        assert vgprs <= want[name][0] and scratch <= want[name][1], (name, (vgprs, scratch), want[name])
