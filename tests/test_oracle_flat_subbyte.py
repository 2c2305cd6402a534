"""CPU: the yardstick of the binary / octal exhaustive scan, pinned without the C.  The oracle's flat search goes through coso_distance,
which is storage-generic; here its candidate stage (flat_candidates_batch: every stored code scored, sorted by score with the larger id
first, cut to 5 * top_k) is restated in numpy — digit dots as integer matrix products, cosine as f32(dot) / (|q| * |v|) in f32 — and the
two must agree id for id, the tie corpus included (tests/flat_subbyte.py)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import flat_subbyte as FS

NQ = 24


@pytest.mark.parametrize("res", [FS.BINARY, FS.OCTAL])
@pytest.mark.parametrize("n,dim", [(4000, 13), (9000, 65)])
def test_candidates_equal_the_numpy_restatement(res, n, dim):
    X, Q = FS.scan_corpus(res, n, dim)
    Q = Q[-NQ:]                                                            # the two uniform queries among them
    ids, cnt, _ = FS.numpy_flat_candidates(X, Q, res, FS.SCAN_K)
    oids, ocnt = FS.oracle_of(X, res).flat_candidates_batch(Q, FS.SCAN_K, threads=4)
    assert np.array_equal(ocnt, cnt) and (ocnt == 5 * FS.SCAN_K).all()
    assert np.array_equal(oids, ids)


@pytest.mark.parametrize("top_k", [10, 60])
def test_tie_corpus_candidates_are_the_largest_ids_of_the_run(top_k):
    X, Q = FS.tie_corpus(nq=NQ)
    ids, cnt, scores = FS.numpy_flat_candidates(X, Q, FS.BINARY, top_k)
    oids, ocnt = FS.oracle_of(X, FS.BINARY).flat_candidates_batch(Q, top_k, threads=4)
    assert np.array_equal(ocnt, cnt) and np.array_equal(oids, ids)
    run = scores[:, FS.TIE_RUN0:]
    assert (run == run[:, :1]).all(), "the run does not tie"
    # the corpus does what it is for: for most queries the run beats every earlier row, and then the answer is the run's largest ids
    wins = run[:, 0] > scores[:, :FS.TIE_RUN0].max(axis=1)
    assert wins.sum() >= NQ // 2
    top = np.arange(FS.TIE_N - 1, FS.TIE_N - 1 - 5 * top_k, -1, dtype=np.uint32)
    assert all(np.array_equal(oids[b], top) for b in np.flatnonzero(wins))


def test_short_binary_rows():
    """the (30001, 24) uniform case of the device test.  A query's integer dots take at most 25 values here, but the cosine divides by the
    norms of the ORIGINAL vectors (the quantizer keeps those for SubByte storage), so equal dots are not equal scores: what this shape
    stresses is many rows a few ulps apart around the cut, not runs of exact ties — those are the tie corpus above"""
    X, Q = FS.uniform_scan_corpus(FS.BINARY, 30001, 24, nq=NQ)
    for top_k in (10, 60):
        ids, cnt, scores = FS.numpy_flat_candidates(X, Q, FS.BINARY, top_k)
        oids, ocnt = FS.oracle_of(X, FS.BINARY).flat_candidates_batch(Q, top_k, threads=4)
        assert np.array_equal(ocnt, cnt) and np.array_equal(oids, ids)


def test_zero_norm_is_the_all_zero_vector_not_the_all_zero_code():
    """SubByte norms are those of the original vector: a row with every component negative has an all-zero binary code and scores 0
    against everything, but only the all-zero VECTOR is a zero norm, i.e. DistanceError::CalculationError (status 2) for an exhaustive scan"""
    X, Q = FS.uniform_scan_corpus(FS.BINARY, 500, 24, nq=8)
    X[17] = -np.abs(X[17])
    oids, osc, ocnt = FS.oracle_of(X, FS.BINARY).flat_search_batch(Q, 5)
    assert (ocnt == 5).all() and not (oids == 17).any()
    X[17] = 0.0
    with pytest.raises(ValueError, match="status 2"):
        FS.oracle_of(X, FS.BINARY).flat_search_batch(Q, 5)
