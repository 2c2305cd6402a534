"""scripts/compare_kernel_code.py on a built object: a build compared with itself is identical (exit status 0), every kernel of
the code object's notes is found in the disassembly, and the budgets are read from the kernel's OWN entry of the notes
(.group_segment_fixed_size comes before .name there)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
LLVM = "/opt/rocm/lib/llvm/bin"


def _object(name):
    src = os.path.join(ROOT, "cosdata_amd", "csrc", name)
    if not os.path.exists(src) or not os.path.exists(os.path.join(LLVM, "llvm-readelf")):
        pytest.skip("built objects / llvm tools not present")
    return src


def test_a_build_is_identical_to_itself(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    for d in (a, b):
        d.mkdir()
        shutil.copy(_object("kernels_order.o"), d)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "compare_kernel_code.py"), str(a), str(b)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "identical" in r.stdout.splitlines()[-1]


def test_budgets_come_from_the_kernels_own_entry(tmp_path):
    import compare_kernel_code as c
    funcs, kernels = c.code_object(LLVM, _object("kernels_sparse.o"), str(tmp_path))
    assert kernels and set(kernels) <= set(funcs)
    wide = [k for k in kernels if "sparse_wide_finish_kernelILi16E" in k]
    assert len(wide) == 1 and kernels[wide[0]]["group_segment_fixed_size"] == 64 * 16 * 8 + 8   # best[1024] + s_ncand, padded to 8
    assert funcs[wide[0]] and all(not i.startswith(("s_branch ", "s_cbranch")) or len(i.split()) == 1 for i in funcs[wide[0]])
