"""cosdata_amd.sharding.slice_row_masks cuts a packed mask over the GLOBAL rows of a sharded collection into one packed mask per shard
over the shard's own rows.  Shard boundaries are generally not multiples of 32, so a shard's words straddle the global ones; checked
against a restatement that moves one bit at a time."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bit(words, r):
    return (int(words[r // 32]) >> (r % 32)) & 1


def _slice_per_bit(bits, bounds):
    out = []
    for lo, hi in zip(bounds, bounds[1:]):
        m = np.zeros((bits.shape[0], (hi - lo + 31) // 32), np.uint32)
        for g in range(bits.shape[0]):
            for j in range(hi - lo):
                if _bit(bits[g], lo + j):
                    m[g, j // 32] |= np.uint32(1 << (j % 32))
        out.append(m)
    return out


BOUNDS = [[0, 37, 64, 65, 200],          # cuts inside a word, on a word, one row wide
          [0, 32, 64, 96],               # word-aligned
          [0, 31, 31, 95, 100],          # an empty shard
          [0, 1, 2, 3, 70],              # one-row shards
          [0, 633, 1266, 1900],          # the ragged thirds of the GPU test's corpus
          [0, 5]]                        # a single shard shorter than a word


@pytest.mark.parametrize("bounds", BOUNDS)
def test_slices_match_the_per_bit_restatement(bounds):
    from cosdata_amd.sharding import slice_row_masks
    rng = np.random.default_rng(len(bounds) * 1000 + bounds[-1])
    N = bounds[-1]
    words = (N + 31) // 32
    bits = rng.integers(0, 2 ** 32, (3, words), dtype=np.uint64).astype(np.uint32)   # bits past N set at random: they must not show
    got = slice_row_masks(bits, bounds)
    exp = _slice_per_bit(bits, bounds)
    assert len(got) == len(bounds) - 1
    for s, (g, e) in enumerate(zip(got, exp)):
        assert g.dtype == np.uint32 and g.shape == e.shape == (3, (bounds[s + 1] - bounds[s] + 31) // 32), (s, g.shape)
        assert np.array_equal(g, e), s
        assert g.flags["C_CONTIGUOUS"]
    # glued back bit by bit, the shards' masks give the original (up to row N)
    for g in range(3):
        glued = [_bit(got[s][g], j) for s in range(len(got)) for j in range(bounds[s + 1] - bounds[s])]
        assert glued == [_bit(bits[g], r) for r in range(N)]


def test_bits_past_the_last_row_are_ignored_and_padding_is_zero():
    from cosdata_amd.sharding import slice_row_masks
    bits = np.full((2, 4), 0xFFFFFFFF, np.uint32)           # 128 bits set, the collection holds 70 rows
    a, b = slice_row_masks(bits, [0, 33, 70])
    assert a.tolist() == [[0xFFFFFFFF, 1]] * 2              # 33 rows: one bit of the second word
    assert b.tolist() == [[0xFFFFFFFF, 0x1F]] * 2           # 37 rows
    one, = slice_row_masks(bits[0], [0, 70])                # a single mask as one row; extra words beyond ceil(N / 32) are accepted
    assert one.tolist() == [[0xFFFFFFFF, 0xFFFFFFFF, 0x3F]]
    empty, full = slice_row_masks(bits, [0, 0, 64])
    assert empty.shape == (2, 0) and full.tolist() == [[0xFFFFFFFF, 0xFFFFFFFF]] * 2


def test_sliced_masks_agree_with_packing_the_sliced_rows():
    """the same cut made on bool rows and packed per shard with the index's own pack_row_masks"""
    from cosdata_amd.index import pack_row_masks
    from cosdata_amd.sharding import slice_row_masks
    rng = np.random.default_rng(3)
    bounds = [0, 633, 1266, 1900]
    m = rng.random((4, 1900)) < 0.3
    got = slice_row_masks(pack_row_masks(m), bounds)
    for s in range(3):
        assert np.array_equal(got[s], pack_row_masks(m[:, bounds[s]:bounds[s + 1]]))


def test_bad_arguments_are_refused():
    from cosdata_amd.sharding import slice_row_masks
    bits = np.zeros((1, 2), np.uint32)
    with pytest.raises(ValueError):
        slice_row_masks(bits, [0, 65])                       # more rows than bits
    with pytest.raises(ValueError):
        slice_row_masks(bits, [0, 40, 30])                   # not ascending
    with pytest.raises(ValueError):
        slice_row_masks(bits.astype(np.int64), [0, 64])      # not the packed layout
    with pytest.raises(ValueError):
        slice_row_masks(bits, [0])


def test_new_entry_points_are_declared_and_mirrored():
    """the header declares the wide merge and the three shard-set calls, and the ctypes table gives each its prototype"""
    hdr = open(os.path.join(ROOT, "include", "cosdata_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib_py = open(os.path.join(ROOT, "cosdata_amd", "_lib.py")).read()
    from cosdata_amd import _lib
    for name in ["cos_merge_lists_device", "cos_merge_lists_packed_device", "cos_shardset_search_filtered_batch", "cos_shardset_flat_search_batch",
                 "cos_shardset_bruteforce_topk"]:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.ABI_SYMBOLS and '"%s": [' % name in lib_py, name
        assert hasattr(_lib.lib(), name), name
    from cosdata_amd.shardset import ShardSet
    for method in ["search_filtered", "flat_search", "bruteforce_topk"]:
        assert callable(getattr(ShardSet, method))
