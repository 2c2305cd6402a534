"""GPU: cos_flat_search_batch over binary (SubByte resolution 1) and octal (resolution 3) codes.  Every assertion is bit-exact against the
oracle's flat_search_batch — counts, ids, score bits — whose candidate stage test_oracle_flat_subbyte.py pins in numpy.  Implementations
compared: the 256 x 128 tile kernel (flat_codes_gemm_i8<ENG_Q1 / ENG_Q3>, unfused score matrix and fused threshold-filtered epilogue) and
the query-resident kernels of kernels_scan.hip (binary: e2m1 digits on the scaled MFMA, and i8 digits under flat_fp4 = 0; octal: i8 digits),
selected by the tuning knobs flat_tile_kernel / flat_unfused / flat_fp4."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import flat_subbyte as FS
from tests import helpers as H
from tests.flat_subbyte import BINARY, OCTAL, SCAN_B, SCAN_K
from tests.test_gpu_append import _device

pytestmark = pytest.mark.gpu

RES = [pytest.param(BINARY, id="binary"), pytest.param(OCTAL, id="octal")]
# (n, dim): below FLAT_SEED, unfused only, a partial last plane byte | two chunks of a plane | a second, fused launch | 769: 7 binary / 13
# octal digit chunks have no query-resident instantiation, the tile kernel runs | 768 and 1023: 12 and 16 digit chunks, query-resident
# kernels, the latter with a partial last chunk
SHAPES = [(4000, 13), (9000, 65), (30001, 129), (40000, 769), (20003, 768), (20003, 1023)]
KNOBS = (dict(flat_tile_kernel=1), dict(flat_unfused=1), dict(flat_fp4=0))


def _index(X, res, metric=None):
    import cosdata_amd as ca
    ix = ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=3), distance_metric=metric or ca.DistanceMetric.Cosine,
                      storage_type=ca.StorageType(ca.StorageKind(O.STORAGE_SUBBYTE), res))
    return ix.upload_vectors(X)


def _oracle(X, Q, res, top_k, metric=O.METRIC_COSINE):
    """the oracle's answer; COSO_OK (anything else raises) and full counts, so that a bad corpus cannot pass for a device bug"""
    ref = FS.oracle_of(X, res, metric).flat_search_batch(Q, top_k, threads=8)
    assert (ref[2] == min(top_k, X.shape[0])).all()
    return ref


def _same(got, ref, B=None, what=None):
    ids, sc, cnt = got[:3]
    oids, osc, ocnt = (a[:B] for a in ref[:3])
    assert np.array_equal(cnt, ocnt), what
    assert np.array_equal(ids, oids), what
    assert np.array_equal(np.ascontiguousarray(sc).view(np.uint32), np.ascontiguousarray(osc).view(np.uint32)), what


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("n,dim", SHAPES)
def test_scan_matches_oracle(res, n, dim):
    from cosdata_amd import _lib
    X, Q = FS.scan_corpus(res, n, dim)
    ref = _oracle(X, Q, res, SCAN_K)                                 # 261 queries; the batches of 5 and 70 are its first rows
    ix = _index(X, res)
    for B in SCAN_B:
        got = ix.flat_search(Q[:B], SCAN_K, with_stats=True)
        _same(got, ref, B, B)
        st = got[3]
        assert st.gemm_launches >= (2 if n > 16384 else 1) and st.gemm_ms > 0
        kdims = {BINARY: (dim + 127) // 128 * 128, OCTAL: ((dim + 31) // 32 * 32 + 63) // 64 * 64}[res]
        assert st.int8_ops == 2.0 * B * n * kdims
        if dim >= 768:
            for knob in KNOBS:
                with _lib.tuning(**knob):
                    _same(ix.flat_search(Q[:B], SCAN_K), ref, B, (B, knob))


def test_octal_odd_chunk_count_on_the_query_resident_kernel():
    """733 octal dims are 23 row chunks of 32: 12 digit chunks of 64, the last of them half absent (ScanRow<ENG_Q3>::load zeroes it)"""
    from cosdata_amd import _lib
    X, Q = FS.scan_corpus(OCTAL, 20003, 733)
    Q = Q[-70:]
    ref = _oracle(X, Q, OCTAL, SCAN_K)
    ix = _index(X, OCTAL)
    _same(ix.flat_search(Q, SCAN_K), ref)
    with _lib.tuning(flat_tile_kernel=1):
        _same(ix.flat_search(Q, SCAN_K), ref, None, "tile kernel")


def test_binary_768_every_form_of_the_fp4_kernel():
    """768 binary dims run flat_scan_q2_fp4_w8<12, 3, ENG_Q1> by default; flat_fp4_w8 = 0 is the one-wave-per-SIMD kernel, 1..3 the other
    orders of the two-wave one (its slot of half a chunk per wave, ScanRow::load_half, from ORDER 1 on)"""
    from cosdata_amd import _lib
    X, Q = FS.scan_corpus(BINARY, 20003, 768)
    ref = _oracle(X, Q, BINARY, SCAN_K)
    ix = _index(X, BINARY)
    for v in (0, 1, 2, 3, 4):
        with _lib.tuning(flat_fp4_w8=v):
            _same(ix.flat_search(Q, SCAN_K), ref, None, v)


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("top_k", [60, 204])
def test_wide_pool(res, top_k):
    """top_k 60: a pool of 512 keys; 204: 1024 keys, the widest"""
    X, Q = FS.scan_corpus(res, 30001, 129)
    Q = Q[-70:]
    _same(_index(X, res).flat_search(Q, top_k), _oracle(X, Q, res, top_k))


@pytest.mark.parametrize("res", RES)
def test_dot_product_metric(res):
    """scores are the converted integer dots: the `metric != 0` arm of the query-resident kernels' screen and of the tile kernel's two epilogues"""
    import cosdata_amd as ca
    from cosdata_amd import _lib
    X, Q = FS.scan_corpus(res, 20003, 768)
    Q = Q[-70:]
    ref = _oracle(X, Q, res, SCAN_K, O.METRIC_DOT)
    ix = _index(X, res, ca.DistanceMetric.DotProduct)
    _same(ix.flat_search(Q, SCAN_K), ref)
    for knob in KNOBS:
        with _lib.tuning(**knob):
            _same(ix.flat_search(Q, SCAN_K), ref, None, knob)


@pytest.mark.parametrize("top_k", [10, 60])
def test_short_binary_rows(top_k):
    """24 binary dims: a query's dots take at most 25 values, so thousands of rows lie within a few ulps of the cut"""
    X, Q = FS.uniform_scan_corpus(BINARY, 30001, 24)
    ix = _index(X, BINARY)
    ref = _oracle(X, Q, BINARY, top_k)
    for B in (70, 261):
        _same(ix.flat_search(Q[:B], top_k), ref, B, B)


def test_ties_overflow_the_append_buffer():
    """rows 16384.. are copies of one vector and the queries are that vector plus noise: every row of the fused chunk ties, and a key passes
    the fused filter when (score, id) beats the threshold KEY, so each later id passes — 13617 appends per query against a capacity of
    4096.  The scan must notice, repeat on the unfused path and return the oracle's lists: the largest ids of the run first.  The handle
    then answers an ordinary batch as it did before."""
    X, Q = FS.tie_corpus(nq=70)
    plain_q = H.queries_from(X[:FS.TIE_RUN0], 20, noise=0.05, seed=9)
    ix = _index(X, BINARY)
    plain = ix.flat_search(plain_q, SCAN_K, with_stats=True)
    _same(plain, _oracle(X, plain_q, BINARY, SCAN_K))
    ref = _oracle(X, Q, BINARY, SCAN_K)
    got = ix.flat_search(Q, SCAN_K, with_stats=True)
    _same(got, ref)
    top = np.arange(FS.TIE_N - 1, FS.TIE_N - 1 - SCAN_K, -1, dtype=np.uint32)
    assert sum(np.array_equal(got[0][b], top) for b in range(Q.shape[0])) >= Q.shape[0] // 2, "the run does not win: the corpus is no test"
    assert got[3].gemm_launches > plain[3].gemm_launches, "the scan was not repeated: the append buffer did not overflow"
    again = ix.flat_search(plain_q, SCAN_K)
    assert all(np.array_equal(a, b) for a, b in zip(plain[:3], again))


def test_zero_norm_is_calculation_error():
    """SubByte storage keeps the norm of the ORIGINAL vector, so the zero norm of these storages is the all-zero vector (a row with every
    component negative is an all-zero binary CODE with a norm: it scores 0 and the call answers, like the oracle's).  A zero-norm stored
    row or query is DistanceError::CalculationError (status 2) for the call; the handle answers afterwards; a re-upload replaces the
    cached flag of the stored vectors"""
    import cosdata_amd as ca
    X, Q = FS.uniform_scan_corpus(BINARY, 20000, 64, nq=6)
    X[17] = -np.abs(X[17])                                           # an all-zero code, not a zero norm
    ix = _index(X, BINARY)
    ok = ix.flat_search(Q, 5)
    _same(ok, _oracle(X, Q, BINARY, 5))
    Qz = Q.copy()
    Qz[3] = 0.0
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search(Qz, 5)
    assert ei.value.status == 2
    again = ix.flat_search(Q, 5)                                     # the flag does not stick to the handle
    assert all(np.array_equal(a, b) for a, b in zip(ok, again))
    X2 = X.copy()
    X2[1234] = 0.0
    with pytest.raises(ValueError, match="status 2"):
        FS.oracle_of(X2, BINARY).flat_search_batch(Q, 5)
    ix.upload_vectors(X2)                                            # a new upload: the cached stored flag must not survive it
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search(Q, 5)
    assert ei.value.status == 2
    ix.upload_vectors(X)                                             # and back
    _same(ix.flat_search(Q, 5), ok)


@pytest.mark.parametrize("kind", [O.STORAGE_F16, O.STORAGE_F32])
def test_float_storages_are_still_refused(kind):
    import cosdata_amd as ca
    X = H.uniform_corpus(2000, 64, seed=5) * np.float32(0.9)
    Q = H.queries_from(X, 9, seed=2)
    ix = ca.HNSWIndex(64, ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType(ca.StorageKind(kind), 0))
    ix.upload_vectors(X)
    with pytest.raises(ca.CosdataError) as ei:
        ix.flat_search(Q, 5)
    assert ei.value.status == 4
    ids, sc = ix.bruteforce_topk(Q, 5)                               # the handle stays usable
    oids, osc = O.bruteforce_topk(X, Q, 5, threads=4)
    assert np.array_equal(ids, oids) and np.array_equal(sc.view(np.uint32), osc.view(np.uint32))


def test_warm_handle_across_append_and_delete():
    """a built binary index that has served a scan, then grows and loses vectors: its scan equals a cold handle's and the oracle's (the
    scan does not filter deleted ids: include/cosdata_hip.h)"""
    n0, add, dim = 3000, 500, 96
    X, Q = FS.uniform_scan_corpus(BINARY, n0 + add, dim, nq=70)
    p = O.HNSWParams(dim=dim, storage=O.STORAGE_SUBBYTE, resolution=BINARY, num_layers=3, ef_construction=32, ef_search=32, seed=11)
    oix = O.OracleIndex(p).set_vectors(X[:n0])
    oix.build_rounds(128)
    dix = _device(X[:n0], p).build(128)
    _same(dix.flat_search(Q, SCAN_K), oix.flat_search_batch(Q, SCAN_K, threads=4))      # warm: workspace and cached flags of 3000 rows
    oix.append(X[n0:], 128)
    dix.append(X[n0:], 128)
    dele = np.random.default_rng(5).permutation(n0 + add)[:40].astype(np.uint32)
    oix.delete(dele)
    dix.delete(dele)
    warm = dix.flat_search(Q, SCAN_K)
    _same(warm, oix.flat_search_batch(Q, SCAN_K, threads=4))
    _same(warm, _index(X, BINARY).flat_search(Q, SCAN_K))
    assert (warm[0] >= n0).any()                                     # appended vectors are found
