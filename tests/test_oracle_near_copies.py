"""The inputs of test_gpu_brute_near_copies.py, checked on the oracle and float64 alone (no GPU): every near-copy corpus really puts
more rows within the scores' error of the k-th score than the survivor pool holds, the exact and power-of-two copies really tie bit
for bit, the scaled ones really do not — and the ordinary test corpora stay far away from all of it.  These are conditions on the
inputs, not measurements of the library: a shape that misses one is the wrong shape."""
import numpy as np
import pytest

from tests import near_copies as NC
from tests import odd_dims as OD


@pytest.mark.parametrize("case", NC.CASES, ids=NC.case_id)
def test_more_rows_near_the_kth_score_than_the_pool_holds(case):
    n, dim, copies, kind, lo_row, k = case
    X, Q, rows = NC.corpus(case)
    assert (rows >= lo_row).all() and len(set(rows.tolist())) == copies
    near = NC.rows_near_kth(X, Q[:NC.AIMED], k)
    print(f"{NC.case_id(case)}: P {NC.pool_width(k)}, rows within 2 * bound_a of the k-th score per aimed query {near.tolist()}")
    assert (near > NC.pool_width(k)).all()


@pytest.mark.parametrize("case", [c for c in NC.CASES if c[3] in ("exact", "pow2")], ids=NC.case_id)
def test_exact_and_pow2_copies_tie_bit_for_bit(case):
    """a power of two scales the dot, both norms and their product exactly: one score, and the tie rule (larger id first) decides"""
    ids, sc = NC.oracle_topk(case)
    for b in range(NC.AIMED):
        assert len(set(sc[b].view(np.uint32).tolist())) == 1, (b, sc[b])
        assert (np.diff(ids[b].astype(np.int64)) < 0).all(), (b, ids[b])
    if case[2] == case[0]:                                   # every row is a copy: ids n-1, n-2, ...
        assert np.array_equal(ids[:NC.AIMED], np.tile(np.arange(case[0] - 1, case[0] - 1 - case[5], -1, dtype=np.uint32), (NC.AIMED, 1)))


@pytest.mark.parametrize("case", [c for c in NC.CASES if c[3] in ("scaled", "mixed") and c[5] > 1], ids=NC.case_id)
def test_scaled_copies_do_not_tie(case):
    """(k = 1 is left out: one entry has one bit pattern.)  The exact order among the copies is then decided by last-ulp differences"""
    _, sc = NC.oracle_topk(case)
    patterns = [len(set(sc[b].view(np.uint32).tolist())) for b in range(NC.AIMED)]
    print(f"{NC.case_id(case)}: distinct score bit patterns in the oracle's top k per aimed query {patterns}")
    assert sum(p >= 2 for p in patterns) >= 6


def test_the_masked_case_keeps_its_conditions_under_the_masks():
    case = NC.MASKED
    X, Q, rows = NC.corpus(case)
    masks = NC.masks_for(case)
    assert (~masks[0][rows]).sum() == case[2] // 2 and masks[0].sum() == case[0] - case[2] // 2
    assert (NC.rows_near_kth(X, Q[:NC.AIMED], case[5], live=masks[0]) > NC.pool_width(case[5])).all()
    assert 0 < masks[1].sum() < case[5] and masks[1][rows].sum() >= case[5] - 5


def test_the_sharded_case_cuts_the_copies_three_ways():
    case = NC.SHARDED
    _, _, rows = NC.corpus(case)
    assert sum(NC.SHARD_SIZES) == case[0]
    bounds = np.concatenate([[0], np.cumsum(NC.SHARD_SIZES)])
    per_shard = [int(((rows >= bounds[s]) & (rows < bounds[s + 1])).sum()) for s in range(3)]
    print(f"copies per shard {per_shard}")
    assert min(per_shard) > case[5]


@pytest.mark.parametrize("shape,ks", NC.ORDINARY, ids=[f"{s[0]}x{s[1]}" for s, _ in NC.ORDINARY])
def test_ordinary_corpora_are_far_from_the_margin(shape, ks):
    """the k-th and the P-th float64 score of every query are more than four times the library's bound apart: with the margin rule at
    twice the bound, no query of these corpora may take the exact path, and the GPU file asserts exactly that"""
    n, dim, B = shape
    X, Q = OD.brute_corpus(n, dim, B)
    for k in ks:
        if NC.pool_width(k) > n:
            continue
        gap = NC.kth_to_pth_gap(X, Q, k)
        print(f"{n} x {dim}, k {k}: smallest gap / bound {gap.min() / NC.margin_bound(dim):.0f}")
        assert (gap > 4.0 * NC.margin_bound(dim)).all()


def test_margin_bound_covers_the_reference_dot():
    """the library's bound is no smaller than bound_a's worst case (sum |x_i q_i| = |x| |q|) at the dims of the cases"""
    for dim in (64, 65, 96, 97, 100, 768):
        assert NC.margin_bound(dim) >= (dim / 8 + 16) * OD.U + 4 * OD.U
