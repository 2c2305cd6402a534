"""Corpora of the binary / octal exhaustive-scan tests (test_gpu_flat_subbyte.py on the device, test_oracle_flat_subbyte.py on the CPU) and a
numpy restatement of the candidate stage of the oracle's flat search for these two storages.

Ties are the stress of these storages: a query's binary dots take at most dim + 1 values (the cosine then divides by the norms of the
original vectors, so equal dots are close scores, not equal ones), and `tie_corpus` ends in a long run of copies of one vector, which
every query scores exactly equally — the fused scan's threshold sits inside that run and each later id beats it."""
import numpy as np

from oracle import oracle as O
from tests import helpers as H

BINARY, OCTAL = 1, 3
SCAN_B = (5, 70, 261)
SCAN_K = 10
NQ = max(SCAN_B)


def _positive_first(A, res):
    """binary: the first component of every row is made positive, so that no row is an all-zero code (at 13 dims one uniform row in 2^13
    is; it would score 0 against everything)"""
    if res == BINARY:
        A[:, 0] = np.abs(A[:, 0]) + np.float32(0.01)
    return A


def scan_corpus(res, n, dim):
    """the corpus and 261 queries of test_gpu_odd_dims._scan_reference, scaled by 0.9, with the binary fix-up"""
    X = (H.uniform_corpus(n, dim, seed=13) if n < 16384 else H.clustered_corpus(n, dim, n_centers=40, sigma=0.2, seed=23)) * np.float32(0.9)
    Q = np.concatenate([H.queries_from(X, NQ - 2, noise=0.05, seed=8), H.uniform_corpus(2, dim, seed=77) * np.float32(0.9)])
    return _positive_first(X, res), _positive_first(Q, res)


def uniform_scan_corpus(res, n, dim, nq=NQ):
    X = H.uniform_corpus(n, dim, seed=29) * np.float32(0.9)
    Q = np.concatenate([H.queries_from(X, nq - 2, noise=0.05, seed=6), H.uniform_corpus(2, dim, seed=78) * np.float32(0.9)])
    return _positive_first(X, res), _positive_first(Q, res)


TIE_N, TIE_DIM, TIE_RUN0 = 30001, 64, 16384


def tie_corpus(nq=70):
    """rows TIE_RUN0.. are copies of one vector v; the queries are v plus small noise.  Every row of the run has the same code, so each
    query scores the whole run equally and (for most queries) above everything before it: the answer is the run's largest ids"""
    X = H.uniform_corpus(TIE_N, TIE_DIM, seed=31) * np.float32(0.9)
    v = H.uniform_corpus(1, TIE_DIM, seed=32)[0] * np.float32(0.9)
    v[0] = abs(v[0]) + np.float32(0.01)
    X[TIE_RUN0:] = v
    Q = (v[None, :] + np.float32(0.02) * np.random.default_rng(33).standard_normal((nq, TIE_DIM))).astype(np.float32)
    return _positive_first(X, BINARY), _positive_first(Q, BINARY)


def oracle_of(X, res, metric=O.METRIC_COSINE):
    return O.OracleIndex(O.HNSWParams(dim=X.shape[1], metric=metric, storage=O.STORAGE_SUBBYTE, resolution=res, num_layers=3)).set_vectors(X)


# ------------------------------------------------------------------------------------------------------------------------------
# numpy restatement (pins the yardstick without the C)
# ------------------------------------------------------------------------------------------------------------------------------
def digits_of(codes, res, dim):
    """plane-major code rows [n][res * ceil(dim / 8)] -> the digits the reference multiplies, [n][8 * ceil(dim / 8)] int64:
    binary the bit, octal p0 + 2 p1 + 4 p2 on the planes as stored (dot_product_binary / dot_product_octal)"""
    pb = (dim + 7) // 8
    planes = np.asarray(codes, np.uint8).reshape(-1, res, pb)
    bits = np.unpackbits(planes, axis=2, bitorder="little").astype(np.int64)         # the bit order cancels: both operands use it
    return sum(bits[:, p, :] << p for p in range(res))


def numpy_flat_candidates(X, Q, res, top_k):
    """ids [B][5 top_k] and counts: f32(integer dot) / (|q| * |v|) in f32 with the quantizer's norms, sorted by (score desc, id desc)"""
    dim = X.shape[1]
    xc, xm = O.quantize_batch(X, O.STORAGE_SUBBYTE, res, -1.0, 1.0)
    qc, qm = O.quantize_batch(Q, O.STORAGE_SUBBYTE, res, -1.0, 1.0)
    assert (xm > 0).all() and (qm > 0).all(), "a zero norm: the corpus is no test of the scan"
    dots = digits_of(qc, res, dim) @ digits_of(xc, res, dim).T
    scores = dots.astype(np.float32) / (qm.astype(np.float32)[:, None] * xm.astype(np.float32)[None, :])
    assert scores.dtype == np.float32
    cap = min(5 * top_k, X.shape[0])
    ids = np.full((Q.shape[0], 5 * top_k), 0xFFFFFFFF, np.uint32)
    idx = np.arange(X.shape[0])
    for b in range(Q.shape[0]):
        order = np.lexsort((-idx, -scores[b].astype(np.float64)))                    # score desc, then id desc
        ids[b, :cap] = order[:cap]
    return ids, np.full(Q.shape[0], cap, np.uint32), scores
