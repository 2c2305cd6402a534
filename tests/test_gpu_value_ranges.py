"""GPU: every dense u8 path under the ranges "auto" quantization can return (tests/value_ranges.py): the benchmark's sampled range, a
tight one and two asymmetric ones, where the codes use all 256 values, a fifth to four fifths of them are 0 or 255, the division of
the quantizer rounds and the scores spread.  Under the default (-1, 1) none of that happens.  Every comparison is bit for bit against
the oracle under the same range: codes, ids, score bits, counts, statuses, adjacency.  What the inputs contain is asserted without a
device in test_oracle_value_ranges.py."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import flat_masked as FM
from tests import helpers as H
from tests import value_ranges as VR
from tests.test_gpu_append import _device
from tests.test_gpu_builder import _assert_same_graph
from tests.test_gpu_parity import WALK_VARIANTS, _assert_same_search, _assert_same_walk, _reset_variant, _set_variant
from tests.test_gpu_walk_table import _same
from tests.test_sharded_merge import _merge_numpy

pytestmark = pytest.mark.gpu

ALL = ["sampled", "tight", "asym_low", "asym_high"]
QUANTIZER_CASES = VR.RANGES + VR.SYMMETRIC + VR.DEGENERATE
METRICS = [("cosine", O.METRIC_COSINE), ("dot", O.METRIC_DOT)]


def _range(X, name):
    (_, lo, hi), = VR.ranges_for(X, (name,))
    return lo, hi


def _u8_index(X, lo, hi, metric=O.METRIC_COSINE, id_base=0):
    """a graph-less device index over X for the exhaustive scans"""
    import cosdata_amd as ca
    ix = ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=3), ca.DistanceMetric(metric), ca.StorageType.UnsignedByte(), (lo, hi), id_base=id_base)
    return ix.upload_vectors(np.ascontiguousarray(X))


def _oracle_scan(X, Q, top_k, lo, hi, metric=O.METRIC_COSINE):
    p = O.HNSWParams(dim=X.shape[1], metric=metric, num_layers=3, range_lo=lo, range_hi=hi)
    return O.OracleIndex(p).set_vectors(np.ascontiguousarray(X)).flat_search_batch(Q, top_k, threads=8)


def _same_answer(got, ref, what):
    assert np.array_equal(got[2], ref[2]), (what, "counts")
    assert np.array_equal(got[0], ref[0]), (what, "ids", np.flatnonzero((got[0] != ref[0]).any(axis=1)))
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), (what, "score bits")


# ---- a. the quantizer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lo,hi", QUANTIZER_CASES, ids=[c[0] for c in QUANTIZER_CASES])
def test_quantizer_equals_the_oracle_on_the_ladder(name, lo, hi):
    """quantize_rows_kernel<ENG_U8> where the quotient sits on an integer and one ulp decides the byte; row widths on both sides of
    the zero padding to 16 bytes; lo == hi and lo > hi, where the quotient is NaN or 1"""
    import cosdata_amd as ca
    differ = 0
    for width in (1, 15, 16, 17, 64, 100):
        x = VR.ladder_rows(lo, hi, width)
        codes, mags = ca.ScalarQuantization.quantize(x, ca.StorageType.UnsignedByte(), (lo, hi))
        ocodes, omags = O.quantize_batch(x, O.STORAGE_U8, 0, lo, hi)
        differ += int(np.count_nonzero(codes != ocodes))
        print(f"{name} width {width}: {int(np.count_nonzero(codes != ocodes))} of {codes.size} bytes differ from the oracle's")
        assert np.array_equal(codes, VR.quantize_u8_numpy(x, lo, hi)), (name, width)
        assert np.array_equal(mags.view(np.uint32), omags.view(np.uint32)), (name, width)
    assert differ == 0, differ


@pytest.mark.parametrize("rname", ALL)
def test_resident_codes_equal_the_oracle(rname):
    """the codes the index holds, root row last; the root is drawn inside the range, so it differs from range to range"""
    X = VR.world("codes", 300, 100)
    lo, hi = _range(X, rname)
    oix = H.oracle_index(X, num_layers=2, ef_construction=16, ef_search=16, range_lo=lo, range_hi=hi)
    dix = H.device_index_from_oracle(oix, X)
    root = oix.root_raw()
    assert lo <= root.min() and root.max() <= hi and np.unique(root).size > 50
    codes, mags = dix.download_codes()
    ocodes, omags = O.quantize_batch(np.vstack([X, root[None, :]]), O.STORAGE_U8, 0, lo, hi)
    assert np.array_equal(np.asarray(codes).reshape(301, -1), ocodes)
    assert np.array_equal(np.asarray(mags).view(np.uint32), omags.view(np.uint32))


# ---- b. every walk kernel ------------------------------------------------------------------------------------------------------------
def _assert_same_statuses(oix, dix, Q, top_k, zero):
    """the launch with the zero-norm query in it: CalculationError for the call, the oracle's statuses, and the oracle's answer for
    every other query, from every walk variant"""
    import cosdata_amd as ca
    oids, osc, ocnt, orc, ostatus = oix.search_batch(Q, top_k, threads=4, raise_on_error=False)
    assert orc == 2 and list(np.flatnonzero(ostatus)) == [zero] and ostatus[zero] == 2
    ok = np.flatnonzero(ostatus == 0)
    for vname, max_b, max_b4, order_min, table in WALK_VARIANTS:
        _set_variant(dix, max_b, max_b4, order_min, table)
        with pytest.raises(ca.CosdataError) as ei:
            dix.batch_search(Q, top_k)
        assert ei.value.status == 2, vname
        ids, sc, cnt, rc, status = dix.batch_search(Q, top_k, return_status=True)
        assert rc == 2 and np.array_equal(status, ostatus), vname
        _same_answer((ids[ok], sc[ok], cnt[ok]), (oids[ok], osc[ok], ocnt[ok]), vname)
    _reset_variant(dix)


def _walk_world(what, n, dim, rname, **kw):
    X = VR.world(what, n, dim)
    lo, hi = _range(X, rname)
    oix = H.oracle_index(X, range_lo=lo, range_hi=hi, **kw)
    dix = H.device_index_from_oracle(oix, X)
    Q = VR.queries(what, X, lo)
    return X, oix, dix, Q


@pytest.mark.parametrize("rname", ALL)
@pytest.mark.parametrize("n,dim", [(2000, 96), (1500, 100)])
def test_every_walk_kernel_equals_the_oracle(n, dim, rname):
    X, oix, dix, Q = _walk_world("walk", n, dim, rname, num_layers=5, ef_construction=64, ef_search=64)
    _assert_same_walk(oix, dix, Q[:-1])
    _assert_same_search(oix, dix, Q[:-1], 10)
    _assert_same_statuses(oix, dix, Q, 10, Q.shape[0] - 1)


# ---- c. the level-table GEMM on full-scale codes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rname", ["sampled", "tight"])
@pytest.mark.parametrize("n,dim", [(4000, 128), (3000, 1024)])
def test_level_table_gemm_on_full_scale_codes(n, dim, rname):
    """level_table_areg with two and with sixteen 64-byte chunks per row: operands a ^ 0x80 over the whole of -128 .. 127, code sums up
    to 255 x dim in the recentring term; the tile kernel (walk_table_gemm = 0), the table-less walk and the oracle give the same bits"""
    import cosdata_amd as ca
    from cosdata_amd import _lib
    X, oix, dix, Q = _walk_world("table", n, dim, rname, num_layers=5, ef_construction=64, ef_search=64)
    dix.set_walk_table(ca.HNSWIndex.WALK_TABLE_AUTO, 1)
    lmin, cols = dix.walk_table_info()
    assert lmin >= 1 and cols > 64, (lmin, cols)
    Qok = np.ascontiguousarray(Q[:-1])
    _assert_same_walk(oix, dix, Qok)
    _assert_same_search(oix, dix, Qok, 10)
    _assert_same_statuses(oix, dix, Q, 10, Q.shape[0] - 1)
    dix.set_walk_table(ca.HNSWIndex.WALK_TABLE_AUTO, 1)
    res = {}
    for gemm in (1, 0):
        with _lib.tuning(walk_table_gemm=gemm):
            res[gemm] = (dix.batch_search(Qok, 10), dix.ann_search_batch(Qok))
            assert dix.last_walk_split().table_evals > 0, gemm
    dix.set_walk_table(0, 0)
    plain = (dix.batch_search(Qok, 10), dix.ann_search_batch(Qok))
    assert dix.last_walk_split().table_evals == 0
    for gemm in (1, 0):
        assert _same(res[gemm][0], plain[0]) and _same(res[gemm][1], plain[1]), gemm
    oids, osc, ocnt = oix.search_batch(Qok, 10, threads=4)[:3]
    _same_answer(res[1][0], (oids, osc, ocnt), "query-resident GEMM")


# ---- d. the pair walk ----------------------------------------------------------------------------------------------------------------
def test_pair_walk_under_the_tight_range():
    """the mixed 301-query launch of test_gpu_walk_pair.py under (-0.025, 0.025): half of the codes saturated, the cached integer dots
    large.  1000 dims, the narrower of that module's two shapes: the pair kernel takes rows of 33 .. 64 sixteen-byte chunks only
    (walk_pair_plan.h, G = 64), and here the last chunk is half padding, zero bytes beside codes that are zero by saturation"""
    from tests import test_gpu_walk_pair as WP
    _, lo, hi = VR.RANGES[0]
    X, oix, dix = WP._graph(1000, 64, 32, (lo, hi))
    assert (oix.params.range_lo, oix.params.range_hi) == (lo, hi) and dix.values_range == (lo, hi)
    WP._pin(dix)
    WP._compare(dix, oix, WP._queries(1000, 64, 32, (lo, hi)), 256, zero=(150,))


def test_pair_walk_knob_at_128_dims_under_the_tight_range():
    """rows of 8 chunks are outside the pair kernel's domain: the same launch with walk_pair = 2 is left to walk_kernel, and both
    answers are the oracle's"""
    from tests import test_gpu_walk_pair as WP
    from tests.test_gpu_walk_table import _check_against_oracle
    _, lo, hi = VR.RANGES[0]
    X, oix, dix = WP._graph(128, 64, 32, (lo, hi))
    WP._pin(dix)
    Q = WP._queries(128, 64, 32, (lo, hi))
    off, rc0, walk0, _, _ = WP._run(dix, Q, 0)
    got, rc, walk, ps, _ = WP._run(dix, Q, 2, 256, taken=False)
    assert rc == rc0 == 2 and _same(got, off) and _same(walk, walk0) and ps.cache_hits == 0
    status = got[3]
    assert list(np.flatnonzero(status)) == [150] and status[150] == 2
    ok = np.flatnonzero(status == 0)
    _check_against_oracle(oix, got[:3], Q, 10, ok[::7])
    WP._check_lists_against_oracle(oix, walk, Q[ok], range(0, ok.size, 23))


# ---- e. the flat code scan, unfused --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rname", ALL)
@pytest.mark.parametrize("mname,metric", METRICS)
def test_flat_code_scan_below_the_seed_chunk(mname, metric, rname):
    X = VR.world("flat", 3001, 100)
    lo, hi = _range(X, rname)
    Q = VR.queries("flat", X, lo)
    got = _u8_index(X, lo, hi, metric).flat_search(Q, 12)
    _same_answer(got, _oracle_scan(X, Q, 12, lo, hi, metric), (mname, rname))


# ---- f. the flat code scan, fused ----------------------------------------------------------------------------------------------------
def _fused_case(dim, metric, rname, top_k):
    from cosdata_amd import _lib
    X = VR.world("fused", 16500, dim)
    lo, hi = _range(X, rname)
    Q = VR.queries("fused", X, lo)
    ix = _u8_index(X, lo, hi, metric)
    ref = _oracle_scan(X, Q, top_k, lo, hi, metric)
    ids, sc, cnt, st = ix.flat_search(Q, top_k, with_stats=True)
    assert st.gemm_launches >= 2                                  # the seed chunk and a fused one
    _same_answer((ids, sc, cnt), ref, "flat_scan_u8_areg")
    for knob in ("flat_tile_kernel", "flat_unfused"):
        with _lib.tuning(**{knob: 1}):
            _same_answer(ix.flat_search(Q, top_k), ref, knob)


@pytest.mark.parametrize("rname", ALL)
@pytest.mark.parametrize("mname,metric", METRICS)
@pytest.mark.parametrize("dim", [128, 1024])
def test_flat_code_scan_fused_chunk(dim, mname, metric, rname):
    """n just above the 16 384-row seed chunk: the threshold screen of the fused epilogue sees scores that spread (a top-1 to top-50
    span of 0.05 .. 0.3, against 0.005 under (-1, 1)); the query-resident kernel, the tile kernel, the score-matrix path, the oracle"""
    _fused_case(dim, metric, rname, 10)


def test_flat_code_scan_fused_chunk_wide_pool():
    """top_k 40: 200 rerank candidates, the pool of 256 keys of kernels_flat_wide.hip"""
    _fused_case(128, O.METRIC_COSINE, "asym_low", 40)


# ---- g. the masked scan --------------------------------------------------------------------------------------------------------------
def test_masked_scan_with_allow_lists_and_deleted_rows():
    from cosdata_amd import _lib
    n, dim, top_k = 16500, 128, 10
    X = VR.world("fused", n, dim)
    lo, hi = _range(X, "asym_low")
    Q = VR.queries("fused", X, lo)
    p = O.HNSWParams(dim=dim, num_layers=3, ef_construction=32, ef_search=32, seed=11, range_lo=lo, range_hi=hi)
    dix = _device(X, p).build(1024)
    full = FM.subset_flat(X, Q, "u8", np.ones(n, bool), top_k, values_range=(lo, hi))
    rng = np.random.default_rng(9)
    top = np.unique(full[0][:20, 0])                              # rows the unmasked scan ranks first, and rows drawn anywhere
    dele = np.sort(np.concatenate([top, np.setdiff1d(rng.choice(n, 80, replace=False), top)[:50 - top.size]])).astype(np.uint32)
    assert dele.size == 50 and np.unique(dele).size == 50
    dix.delete(dele)
    gone = np.zeros(n, bool)
    gone[dele] = True
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.1])
    qm = np.arange(Q.shape[0], dtype=np.uint32) % 2
    refs = [FM.subset_flat(X, Q, "u8", masks[g] & ~gone, top_k, values_range=(lo, hi)) for g in range(2)]
    ref = tuple(np.stack([refs[qm[b]][a][b] for b in range(Q.shape[0])]) for a in range(3))
    assert FM.mask_matters(full[0], masks[0] & ~gone) == Q.shape[0]
    FM.same(dix.flat_search_masked(Q, top_k, masks, qm, skip_deleted=True), ref, what="default")
    for knob in (dict(flat_tile_kernel=1), dict(flat_unfused=1)):
        with _lib.tuning(**knob):
            FM.same(dix.flat_search_masked(Q, top_k, masks, qm, skip_deleted=True), ref, what=knob)
    FM.same(dix.flat_search_masked(Q, top_k, skip_deleted=True), FM.subset_flat(X, Q, "u8", ~gone, top_k, values_range=(lo, hi)), what="skip_deleted alone")


# ---- h. builder and append -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rname", ["sampled", "asym_low"])
def test_build_and_append_equal_the_oracle(rname):
    n0, add, dim, batch = 1500, 300, 96, 64
    X = VR.world("builder", n0 + add, dim)
    lo, hi = _range(X, rname)
    p = O.HNSWParams(dim=dim, num_layers=5, ef_construction=64, ef_search=64, seed=77, range_lo=lo, range_hi=hi)
    oix = O.OracleIndex(p).set_vectors(X[:n0]).build_rounds(batch, greedy=False)[0]
    dix = _device(X[:n0], p).build(batch)
    _assert_same_graph(dix, oix)                                   # (the root as well: both draw it inside the range)
    root = oix.root_raw()
    assert lo <= root.min() and root.max() <= hi

    def same_codes(rows):
        codes, mags = dix.download_codes()
        ocodes, omags = O.quantize_batch(np.vstack([X[:rows], root[None, :]]), O.STORAGE_U8, 0, lo, hi)
        assert np.array_equal(np.asarray(codes).reshape(rows + 1, -1), ocodes) and np.array_equal(ocodes, oix.codes())
        assert np.array_equal(np.asarray(mags).view(np.uint32), omags.view(np.uint32)) and np.array_equal(omags.view(np.uint32), oix.mags().view(np.uint32))

    same_codes(n0)
    oix.append(X[n0:], batch)
    dix.append(X[n0:], batch)
    assert dix.n == n0 + add
    _assert_same_graph(dix, oix)
    same_codes(n0 + add)
    Q = VR.queries("builder", X, lo)
    _assert_same_walk(oix, dix, Q[:-1])
    _assert_same_search(oix, dix, Q[:-1], 10)
    _assert_same_statuses(oix, dix, Q, 10, Q.shape[0] - 1)
    assert (dix.batch_search(Q[:-1], 10)[0] >= n0).any()           # appended rows are found


# ---- i. the shard set ----------------------------------------------------------------------------------------------------------------
def test_shard_set_flat_search_is_the_per_shard_oracle_scan_merged():
    from cosdata_amd.shardset import ShardSet
    sizes, top_k = [1033, 900, 1067], 10                            # ragged: no boundary is a multiple of 32
    X = VR.world("shards", 3000, 96)
    lo, hi = _range(X, "asym_high")
    Q = VR.queries("shards", X, lo)
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    shards = [_u8_index(X[bounds[s]:bounds[s + 1]], lo, hi, id_base=int(bounds[s])) for s in range(3)]
    parts = []
    for s in range(3):
        ids, sc, cnt = _oracle_scan(X[bounds[s]:bounds[s + 1]], Q, top_k, lo, hi)
        assert (cnt == top_k).all()
        parts.append(((ids + np.uint32(bounds[s])).astype(np.uint32), sc, cnt))
    exp = _merge_numpy(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]).astype(np.uint32), top_k)
    ss = ShardSet(shards)
    got = ss.flat_search(Q, top_k)
    _same_answer(got, exp, "shard set")
    assert len({int(np.searchsorted(bounds[1:], i, side="right")) for i in got[0].ravel()}) == 3      # every shard contributes
    ss.close()
