"""No GPU: the Python mirror of cos_scan_mask equals the header's layout, and the mask packing is the layout the header states — bit
(r % 32) of word r / 32 is row r, little-endian within a word, padding bits clear."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_mask_struct_layout_matches_header(tmp_path):
    from cosdata_amd import _lib
    from cosdata_amd._lib import CosScanMask
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cosdata_hip.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu %zu %u\\n", sizeof(cos_scan_mask), offsetof(cos_scan_mask, struct_size), '
                   'offsetof(cos_scan_mask, flags), offsetof(cos_scan_mask, n_masks), offsetof(cos_scan_mask, bits), '
                   'offsetof(cos_scan_mask, query_mask), COS_SCAN_SKIP_DELETED);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sz, o_size, o_flags, o_n, o_bits, o_qm, skip = map(int, subprocess.check_output([str(exe)]).split())
    assert C.sizeof(CosScanMask) == sz == 32
    assert (CosScanMask.struct_size.offset, CosScanMask.flags.offset, CosScanMask.n_masks.offset) == (o_size, o_flags, o_n) == (0, 4, 8)
    assert (CosScanMask.bits.offset, CosScanMask.query_mask.offset) == (o_bits, o_qm) == (16, 24)
    assert _lib.SCAN_SKIP_DELETED == skip == 1
    hdr = open(os.path.join(ROOT, "include", "cosdata_hip.h")).read()
    assert re.search(r"#define\s+COS_SCAN_SKIP_DELETED\s+1u", hdr)


def test_mask_packing_is_little_endian_within_a_word():
    from cosdata_amd.index import pack_row_masks
    n = 20003
    rng = np.random.default_rng(5)
    masks = np.stack([rng.random(n) < 0.5, np.zeros(n, bool), np.ones(n, bool)])
    bits = pack_row_masks(masks)
    words = (n + 31) // 32
    assert bits.dtype == np.uint32 and bits.shape == (3, words) and bits.flags["C_CONTIGUOUS"]
    for g in range(3):
        for r in (0, 1, 31, 32, 33, 16383, 16384, n - 1):
            assert bool((int(bits[g, r // 32]) >> (r % 32)) & 1) == bool(masks[g, r]), (g, r)
        back = np.array([(int(bits[g, r // 32]) >> (r % 32)) & 1 for r in range(n)], bool)
        assert np.array_equal(back, masks[g])
        assert int(bits[g, -1]) >> (n % 32) == 0                      # rows n .. 32 * words - 1 do not exist: clear
    one = pack_row_masks(np.arange(40) == 33)                         # a single mask [n] is a [1][n] set
    assert one.shape == (1, 2) and one[0, 0] == 0 and one[0, 1] == 2
    assert pack_row_masks(np.ones((2, 64), bool)).tolist() == [[0xFFFFFFFF] * 2] * 2   # n a multiple of 32: no padding word
