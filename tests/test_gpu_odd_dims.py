"""GPU: every kernel at dimensions that are NOT a multiple of four — odd, below 16, one off a power of two, one off a 64-byte chunk.
What exists only for these dimensions: the scalar tails of f32_pair_dot / f32_oct_dot / f16_lane_dot (dot_engines.h), raw rows that
are only 4-byte aligned (raw_stride = dim), flat_gemm_f32<false, *> (the non-float4 staging of cos_bruteforce_topk), the final partial
byte of a SubByte plane and its place in the device layout, u8 rows padded to 16 bytes, G = pow2ceil(1..3 chunks), and the dispatch
fall-backs next to the kernels that take whole 64-byte chunks only.  Everything is compared bit for bit with the oracle through the
C ABI (the oracle itself is pinned at these dimensions by test_oracle_odd_dims.py); the f32 / f16 / u8 rerank scores and the brute
force are also held to the float64 cosine of the raw vectors, which does not pass through the oracle (tests/odd_dims.py)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import meta_helpers as MH
from tests import odd_dims as OD
from tests.odd_dims import D, STORAGES, WALK_DIMS
from tests.test_gpu_append import _device, _same_graph
from tests.test_gpu_meta import _assert_same_filtered
from tests.test_gpu_parity import _assert_same_search, _assert_same_walk

pytestmark = pytest.mark.gpu

FLOAT64_CHECKED = (O.STORAGE_U8, O.STORAGE_F16, O.STORAGE_F32)       # the rerank is the f32 cosine of the RAW vectors for every storage


def _stype(storage, res):
    import cosdata_amd as ca
    return ca.StorageType(ca.StorageKind(storage), res)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------
# operators
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,storage,res", STORAGES)
@pytest.mark.parametrize("dim", D)
def test_quantize_batch(name, storage, res, dim):
    import cosdata_amd as ca
    x = np.random.default_rng(dim).uniform(-1.3, 1.3, (37, dim)).astype(np.float32)
    sp = np.array([1.0, -1.0, np.nan, 5e30], np.float32)            # wrap / saturate / NaN / huge (test_quantize_matches_oracle)
    x[0, :min(4, dim)] = sp[:min(4, dim)]
    x[1, :] = 0.0
    x[2, 0], x[3, 0], x[4, dim - 1], x[5, dim // 2], x[6, dim - 1] = sp[0], sp[1], sp[2], sp[3], sp[0]
    codes, mags = ca.ScalarQuantization.quantize(x, _stype(storage, res), (-1.0, 1.0))
    ocodes, omags = O.quantize_batch(x, storage, res, -1.0, 1.0)
    assert np.array_equal(codes, ocodes)
    assert _same_bits(mags, omags)
    if storage == O.STORAGE_SUBBYTE and dim % 8:
        assert not (np.asarray(codes).reshape(37, res, -1)[:, :, -1] >> (dim % 8)).any(), "bits past dim in a plane's final byte"


@pytest.mark.parametrize("name,storage,res", STORAGES)
@pytest.mark.parametrize("dim", [3, 13, 33, 65, 129, 257])
def test_resident_codes(name, storage, res, dim):
    """cos_index_download_codes: device layout (16-byte chunks of interleaved planes, padded u8 rows) -> reference layout"""
    X = H.uniform_corpus(300, dim, seed=17) * 1.1
    oix = H.oracle_index(X, storage, res, num_layers=2, ef_construction=16, ef_search=16)
    dix = H.device_index_from_oracle(oix, X)
    codes, mags = dix.download_codes()
    ocodes, omags = O.quantize_batch(np.vstack([X, oix.root_raw()[None, :]]), storage, res, -1.0, 1.0)
    assert np.array_equal(np.asarray(codes).reshape(301, -1), np.ascontiguousarray(ocodes).view(np.uint8).reshape(301, -1))
    assert _same_bits(mags, omags)


@pytest.mark.parametrize("name,storage,res", STORAGES)
@pytest.mark.parametrize("dim", [1, 3, 7, 13, 17, 33, 65, 129, 257, 1023])
def test_distance_batch(name, storage, res, dim):
    """cos_distance_batch, four metrics, the status arms included; every row is an x and a y of some pair, a zero-norm row among them"""
    import cosdata_amd as ca
    nrow = 16
    x = np.random.default_rng(17 + dim).uniform(-1.2, 1.2, (nrow, dim)).astype(np.float32)
    x[3] = 0.0                                                       # zero norm: SubByte, f16, f32
    x[4] = -1.0                                                      # zero norm: u8 (all-zero code)
    stype = _stype(storage, res)
    codes, mags = ca.ScalarQuantization.quantize(x, stype, (-1.0, 1.0))
    ocodes, omags = O.quantize_batch(x, storage, res, -1.0, 1.0)
    assert np.array_equal(codes, ocodes) and _same_bits(mags, omags)
    px, py = [a.ravel().astype(np.uint32) for a in np.meshgrid(np.arange(nrow), np.arange(nrow), indexing="ij")]
    seen = set()
    for metric in (O.METRIC_COSINE, O.METRIC_EUCLIDEAN, O.METRIC_HAMMING, O.METRIC_DOT):
        vals, status = ca.distance_batch(ca.DistanceMetric(metric), stype, dim, codes, mags, codes, mags, px, py)
        for p in range(px.size):
            rc, v = O.distance(metric, storage, res, dim, ocodes[px[p]], omags[px[p]], ocodes[py[p]], omags[py[p]])
            assert status[p] == rc, (name, metric, p, status[p], rc)
            seen.add(rc)
            if rc == 0:
                assert np.float32(vals[p]).tobytes() == np.float32(v).tobytes() or (np.isnan(vals[p]) and np.isnan(v)), (name, metric, p, vals[p], v)
    assert 0 in seen and 2 in seen                                   # values and the CalculationError arm were both compared


# ------------------------------------------------------------------------------------------------------------------------------
# walk + rerank
# ------------------------------------------------------------------------------------------------------------------------------
def _walk_and_search(oix, dix, X, Q, storage, efs=(32, 200)):
    for ef in efs:                                                   # 200: the pool wider than 128 keys
        oix.set_ef_search(ef)
        dix.set_ef_search(ef)
        _assert_same_walk(oix, dix, Q)
        _assert_same_search(oix, dix, Q, 10)
        _assert_same_search(oix, dix, Q, 5)
        if storage in FLOAT64_CHECKED:
            ids, sc, cnt = dix.batch_search(Q, 10)
            OD.assert_scores_within_bound(X, Q, ids, sc, cnt, what=f"rerank ef {ef}")
    _assert_one_wave_finalize(oix, dix, Q)


def _has_level_table(storage, res, dim):
    """the level table's domain (level_table_eng_supported, kernels_flat.hip): u8 codes of any length; quaternary codes whose 16-byte
    chunks (64 dimensions each, the last one partial) number 2, 4, 6, 8, 12 or 16 (flat_scan_supported, kernels_scan.hip)"""
    return storage == O.STORAGE_U8 or (storage == O.STORAGE_SUBBYTE and res == 2 and (dim + 63) // 64 in (2, 4, 6, 8, 12, 16))


def _assert_table_path(dix, Q, storage, res, dim):
    """which path the level-table walk variants took: inside the table's domain the table must exist and a throughput-kernel launch
    must read it; outside it (binary, octal, f16, f32, quaternary rows of another chunk count) none may be reported"""
    n_upper = sum(dix.level_count(l) for l in range(1, dix.hnsw_params.num_layers + 1))
    dix.set_latency_mode(0)                                          # the one-wave latency kernel reads no table
    dix.set_latency_waves(0)
    want = (1, n_upper) if _has_level_table(storage, res, dim) else (0, 0)
    assert dix.walk_table_info() == want
    dix.batch_search(Q, 10)
    sp = dix.last_walk_split()
    if want[0]:
        assert sp.table_level_min == 1 and sp.table_cols == n_upper and sp.table_evals > 0, "the level table did not run"
    else:
        assert sp.table_level_min == 0 and sp.table_evals == 0, "a level table ran outside its domain"
    import cosdata_amd as ca
    dix.set_latency_mode(ca.HNSWIndex.LATENCY_MODE_DEFAULT_MAX_B)
    dix.set_latency_waves(ca.HNSWIndex.LATENCY_WAVES_DEFAULT_MAX_B)


def _assert_one_wave_finalize(oix, dix, Q):
    """Launches of up to 1024 queries rerank with eight waves per query (rerank_wide: f32_oct_dot, dword loads).  Bigger launches take
    the one-wave kernels, whose rerank is f32_pair_dot: 16-byte loads from raw rows that are only 4-byte aligned once dim % 4 != 0, and
    the pair version of the scalar tail.  finalize_wide_max_b = 0 sends a small launch there: finalize_fast_kernel<1> (+ the list
    kernel), with finalize_fast = 0 finalize_kernel<FR> — its one-sort branch (5k <= 64 survivors) and, at top_k 20, the blocked one."""
    from cosdata_amd import _lib
    for top_k in (10, 20):
        oids, osc, ocnt = oix.search_batch(Q, top_k, threads=4)[:3]
        for knobs in (dict(finalize_wide_max_b=0), dict(finalize_wide_max_b=0, finalize_fast=0)):
            with _lib.tuning(**knobs):
                ids, sc, cnt = dix.batch_search(Q, top_k)
            assert np.array_equal(cnt, ocnt), (top_k, knobs)
            for b in range(Q.shape[0]):
                c = int(cnt[b])
                assert np.array_equal(ids[b, :c], oids[b, :c]) and _same_bits(sc[b, :c], osc[b, :c]), (top_k, knobs, b)


@pytest.mark.parametrize("name,storage,res", STORAGES)
@pytest.mark.parametrize("dim", WALK_DIMS)
def test_walk_and_rerank(name, storage, res, dim):
    for kind in ("uniform", "clustered"):
        X = OD.walk_corpus(kind, 1200, dim, storage)
        Q = OD.walk_queries(X, dim, storage)
        oix = H.oracle_index(X, storage, res, num_layers=4, ef_construction=32, ef_search=32)
        dix = H.device_index_from_oracle(oix, X)
        _assert_table_path(dix, Q, storage, res, dim)                # u8: every dim; quaternary: 65, 127 and 255 (2 or 4 chunks)
        _walk_and_search(oix, dix, X, Q, storage)


@pytest.mark.parametrize("name,storage,res", [STORAGES[0], STORAGES[2]])
@pytest.mark.parametrize("dim", [769, 1023])
def test_walk_with_the_level_table_on_rows_that_are_no_whole_chunks(name, storage, res, dim):
    """769 and 1023 with the level table on.  u8: level_table_areg takes rows of whole 64-byte chunks only, so the table comes from
    the tile kernel whatever walk_table_gemm says.  Quaternary: a table exists where the row's 16-byte chunks (64 dimensions each, the
    last one partial) number 2, 4, 6, 8, 12 or 16 (flat_scan_supported, kernels_scan.hip) — 1023 dimensions fill 16 chunks and take
    level_table_areg<16> or the tile kernel, 769 fill 13 and walk rows.  Which of the two ran is asserted, and every answer must be
    the table-less walk's and the oracle's."""
    from cosdata_amd import _lib
    X = OD.walk_corpus("clustered", 2000, dim, storage)
    Q = np.concatenate([OD.walk_queries(X, dim, storage), H.queries_from(X, 58, noise=0.05, seed=21)])
    oix = H.oracle_index(X, storage, res, num_layers=4, ef_construction=32, ef_search=32)
    dix = H.device_index_from_oracle(oix, X)
    dix.set_latency_mode(0)                                          # the one-wave latency kernel reads no table
    dix.set_latency_waves(0)
    has_table = _has_level_table(storage, res, dim)
    lmin, cols = dix.walk_table_info()
    assert (lmin, cols) == ((1, sum(dix.level_count(l) for l in range(1, 5))) if has_table else (0, 0))
    res_t = {}
    for gemm in (1, 0):
        with _lib.tuning(walk_table_gemm=gemm):
            res_t[gemm] = (dix.batch_search(Q, 10), dix.ann_search_batch(Q))
            sp = dix.last_walk_split()
            if has_table:
                assert sp.table_level_min == 1 and sp.table_cols == cols and sp.table_evals > 0, "the level table did not run"
            else:
                assert sp.table_level_min == 0 and sp.table_evals == 0, "a level table ran outside its domain"
    dix.set_walk_table(0, 0)
    plain = (dix.batch_search(Q, 10), dix.ann_search_batch(Q))
    assert dix.last_walk_split().table_evals == 0
    for gemm in (1, 0):
        for got, ref in zip(tuple(res_t[gemm][0]) + tuple(res_t[gemm][1]), tuple(plain[0]) + tuple(plain[1])):
            assert _same_bits(got, ref), gemm
    _walk_and_search(oix, dix, X, Q[:16], storage)                   # every variant, the table ones among them, against the oracle


@pytest.mark.parametrize("dim", [2049, 4095, 4099])
def test_walk_wide_u8_rows(dim):
    """2049: the first dimension of three chunk passes in walk_kernel, 4095: the last row shorter than four full passes, 4099: the
    first rows of walk_general_kernel that are no multiple of four"""
    X = H.clustered_corpus(1200, dim, n_centers=8, seed=dim)
    Q = H.queries_from(X, 7, seed=2)
    oix = H.oracle_index(X, O.STORAGE_U8, 0, num_layers=3, ef_construction=32, ef_search=32)
    dix = H.device_index_from_oracle(oix, X)
    _walk_and_search(oix, dix, X, Q, O.STORAGE_U8)


# ------------------------------------------------------------------------------------------------------------------------------
# dim = 1: every cosine is +-1
# ------------------------------------------------------------------------------------------------------------------------------
def test_dim1_u8_build_and_search_statuses():
    """a u8 corpus of one dimension holds all-zero codes (x < -1 + 2/255): the build meets a zero norm -> CalculationError, from
    the device as from the oracle; without such a row the index builds and a zero-norm QUERY fails alone"""
    import cosdata_amd as ca
    X = H.uniform_corpus(400, 1, seed=42)
    X[17] = -1.0
    p = O.HNSWParams(dim=1, num_layers=3, ef_construction=24, ef_search=24, seed=5)
    with pytest.raises(ValueError, match="status 2"):
        O.OracleIndex(p).set_vectors(X).build()
    with pytest.raises(ValueError, match="status 2"):
        O.OracleIndex(p).set_vectors(X).build_rounds(64)
    with pytest.raises(ca.CosdataError) as ei:
        _device(X, p).build(64)
    assert ei.value.status == 2
    X[X < -0.98] = 0.5
    oix = O.OracleIndex(p).set_vectors(X)
    oix.build_rounds(64)
    dix = _device(X, p).build(64)
    _same_graph(dix.download_graph(), oix.export_graph())
    Q = np.array([[0.3], [-0.4], [-1.0], [0.9]], np.float32)
    o = oix.search_batch(Q, 5, raise_on_error=False)
    ids, sc, cnt, rc, status = dix.batch_search(Q, 5, return_status=True)
    assert rc == 2 and o[3] == 2
    assert np.array_equal(status, o[4]) and list(status) == [0, 0, 2, 0]
    good = np.array([0, 1, 3])
    assert np.array_equal(cnt[good], o[2][good]) and np.array_equal(ids[good], o[0][good]) and _same_bits(sc[good], o[1][good])


@pytest.mark.parametrize("name,storage,res", STORAGES[1:])
def test_dim1_all_ties(name, storage, res):
    """all scores tie at +-1: the order is the larger-id rule alone"""
    X = OD.walk_corpus("uniform", 400, 1, storage)
    Q = OD.walk_queries(X, 1, storage, nq=8)
    oix = H.oracle_index(X, storage, res, num_layers=3, ef_construction=24, ef_search=24)
    dix = H.device_index_from_oracle(oix, X)
    _assert_same_walk(oix, dix, Q)
    _assert_same_search(oix, dix, Q, 10)
    ids, sc, cnt = dix.batch_search(Q, 10)
    for b in range(Q.shape[0]):
        c = max(int(cnt[b]), 1)
        ties = np.flatnonzero(sc[b, :c - 1].view(np.uint32) == sc[b, 1:c].view(np.uint32))
        assert (ids[b, ties] > ids[b, ties + 1]).all(), f"query {b}: equal scores are not ordered by the larger id"


# ------------------------------------------------------------------------------------------------------------------------------
# brute force: flat_gemm_f32<false, false> (seed chunk) and <false, true> (fused chunks past 16384 candidates)
# ------------------------------------------------------------------------------------------------------------------------------
def _check_bruteforce(X, Q, ids, sc, k):
    oids, osc = O.bruteforce_topk(X, Q, k, threads=8)
    assert np.array_equal(ids, oids)
    assert _same_bits(sc, osc)
    OD.assert_scores_within_bound(X, Q, ids, sc, what="bruteforce")
    assert OD.float64_topk_excused(X, Q, ids, k) <= 0.05 * Q.shape[0]


@pytest.mark.parametrize("n,dim,B,k", OD.BRUTE_CASES)
def test_bruteforce_unaligned_rows(n, dim, B, k):
    import cosdata_amd as ca
    X, Q = OD.brute_corpus(n, dim, B)
    ix = ca.HNSWIndex(dim, ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType.UnsignedByte())
    ix.upload_vectors(X)
    ids, sc = ix.bruteforce_topk(Q, k)
    _check_bruteforce(X, Q, ids, sc, k)


def test_bruteforce_borrowed_table_off_by_one_float():
    """dim % 4 == 0, but the borrowed table starts 4 bytes past a 16-byte boundary: the second way into the non-float4 staging"""
    import torch
    import cosdata_amd as ca
    n, dim, B, k = OD.BRUTE_BORROWED
    X, Q = OD.brute_corpus(n, dim, B)
    buf = torch.empty(n * dim + 1, dtype=torch.float32, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:]
    view.copy_(torch.from_numpy(X).reshape(-1))
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 == 4
    ix = ca.HNSWIndex(dim, ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType.UnsignedByte())
    ix.upload_vectors_device(view.data_ptr(), n, keepalive=buf)
    ids, sc = ix.bruteforce_topk(Q, k)
    _check_bruteforce(X, Q, ids, sc, k)


# ------------------------------------------------------------------------------------------------------------------------------
# code scan
# ------------------------------------------------------------------------------------------------------------------------------
SCAN_SHAPES = [(4000, 13), (9000, 65), (30001, 129), (40000, 769), (20003, 1023)]
SCAN_B = [5, 70, 261]
SCAN_K = 10


def _scan_reference(storage, res, n, dim):
    """the corpus, 261 queries and the oracle's answer for all of them: the oracle answers query by query, so the batches of 5 and
    70 are the first rows of the same reference"""
    X = (H.uniform_corpus(n, dim, seed=13) if n < 16384 else H.clustered_corpus(n, dim, n_centers=40, sigma=0.2, seed=23)) * np.float32(0.9)
    Q = np.concatenate([H.queries_from(X, max(SCAN_B) - 2, noise=0.05, seed=8), H.uniform_corpus(2, dim, seed=77) * np.float32(0.9)])
    oix = O.OracleIndex(O.HNSWParams(dim=dim, storage=storage, resolution=res, num_layers=3)).set_vectors(X)
    ref = oix.flat_search_batch(Q, SCAN_K, threads=8)
    return X, Q, ref


@pytest.mark.parametrize("name,storage,res", [STORAGES[0], STORAGES[2]])
@pytest.mark.parametrize("n,dim", SCAN_SHAPES)
def test_flat_code_scan(name, storage, res, n, dim):
    """cos_flat_search_batch: u8 rows that are no whole 16-byte chunk, quaternary planes with a partial last byte.  The query-resident
    kernels take whole 64-byte chunks only: u8 rows of 769 and 1023 dimensions (row_stride 784 / 1024 against dim) and quaternary rows
    of 769 (13 chunks) fall back to the tile kernel, quaternary rows of 1023 fill 16 chunks and stay on flat_scan_q2_areg / the FP4
    kernel with a partial last chunk.  Both wide cases must give the same answer under flat_tile_kernel and flat_unfused too."""
    import cosdata_amd as ca
    from cosdata_amd import _lib
    X, Q, (oids, osc, ocnt) = _scan_reference(storage, res, n, dim)
    ix = ca.HNSWIndex(dim, ca.HNSWHyperParams(num_layers=3), storage_type=_stype(storage, res))
    ix.upload_vectors(X)
    for B in SCAN_B:
        ids, sc, cnt, st = ix.flat_search(Q[:B], SCAN_K, with_stats=True)
        assert np.array_equal(cnt, ocnt[:B]) and np.array_equal(ids, oids[:B]) and _same_bits(sc, osc[:B]), B
        assert st.gemm_launches >= (2 if n > 16384 else 1)
        if dim in (769, 1023):
            for knob in ("flat_tile_kernel", "flat_unfused"):
                with _lib.tuning(**{knob: 1}):
                    got = ix.flat_search(Q[:B], SCAN_K)
                assert np.array_equal(got[2], ocnt[:B]) and np.array_equal(got[0], oids[:B]) and _same_bits(got[1], osc[:B]), (B, knob)


# ------------------------------------------------------------------------------------------------------------------------------
# build, append, delete
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,storage,res", [STORAGES[0], STORAGES[2], STORAGES[5], STORAGES[3]])
@pytest.mark.parametrize("dim", [13, 65])
def test_build_append_delete(name, storage, res, dim):
    n0, add = 1500, 300
    X = H.clustered_corpus(n0 + add, dim, n_centers=20, seed=dim + n0) * np.float32(OD.scale_of(storage))
    p = O.HNSWParams(dim=dim, storage=storage, resolution=res, num_layers=4, ef_construction=48, ef_search=40, seed=11)
    oix = O.OracleIndex(p).set_vectors(X[:n0])
    oix.build_rounds(128)
    dix = _device(X[:n0], p).build(128)
    _same_graph(dix.download_graph(), oix.export_graph())
    oix.append(X[n0:], 128)
    dix.append(X[n0:], 128)
    assert dix.n == n0 + add and dix.level_count(0) == n0 + add + 1
    _same_graph(dix.download_graph(), oix.export_graph())
    dele = np.random.default_rng(5).permutation(n0 + add)[:40].astype(np.uint32)
    oix.delete(dele)
    dix.delete(dele)
    _same_graph(dix.download_graph(), oix.export_graph())
    Q = np.concatenate([H.queries_from(X[n0:], 60, noise=0.05, seed=3), X[dele[:20]]])
    ids, sc, cnt = dix.batch_search(Q, 10)
    oids, osc, ocnt = oix.search_batch(Q, 10, threads=4)[:3]
    assert np.array_equal(cnt, ocnt) and np.array_equal(ids, oids) and _same_bits(sc, osc)
    assert (ids[:60] >= n0).any()                                    # appended vectors are found


# ------------------------------------------------------------------------------------------------------------------------------
# filtered walk
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,res,dim", [(O.STORAGE_U8, 0, 33), (O.STORAGE_SUBBYTE, 2, 65)])
def test_filtered_search(storage, res, dim):
    sc = MH.Scenario(n=1500, dim=dim, seed=4, storage=storage, res=res)
    oix = sc.oracle()
    dix = sc.device(oix)
    Q, off, rows, desc = sc.queries(nq=36, seed=7)
    gi, gc = _assert_same_filtered(sc, oix, dix, Q, off, rows, 10)
    assert (gc > 0).sum() >= 18                                      # is / and / or filters do find their replicas
    oix.set_ef_search(200)
    dix.set_ef_search(200)
    _assert_same_filtered(sc, oix, dix, Q[:12], off[:13], rows[:off[12]], 5)
