"""GPU parity: the HIP path (through the C ABI) must match the oracle bit-exactly on identical inputs."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.gpu

STORAGES = [
    ("u8", O.STORAGE_U8, 0),
    ("q2", O.STORAGE_SUBBYTE, 2),
    ("f32", O.STORAGE_F32, 0),
    ("f16", O.STORAGE_F16, 0),
    ("bin", O.STORAGE_SUBBYTE, 1),
    ("oct", O.STORAGE_SUBBYTE, 3),
]


@pytest.mark.parametrize("name,storage,res", STORAGES)
@pytest.mark.parametrize("dim", [96, 100, 768])
def test_quantize_matches_oracle(name, storage, res, dim):
    import cosdata_amd as ca
    rng = np.random.default_rng(1)
    x = rng.uniform(-1.3, 1.3, (37, dim)).astype(np.float32)
    x[0, :4] = [1.0, -1.0, np.nan, 5e30]  # wrap / saturate / NaN / huge quirks (SURVEY App. C 1,4)
    x[1, :] = 0.0
    codes, mags = ca.ScalarQuantization.quantize(x, ca.StorageType(ca.StorageKind(storage), res), (-1.0, 1.0))
    ocodes, omags = O.quantize_batch(x, storage, res, -1.0, 1.0)
    assert np.array_equal(codes, ocodes)
    assert np.array_equal(mags.view(np.uint32), omags.view(np.uint32))


@pytest.mark.parametrize("name,storage,res", STORAGES)
@pytest.mark.parametrize("dim", [100, 768])
def test_resident_codes_match_oracle(name, storage, res, dim):
    """cos_index_download_codes: the codes the index holds in HBM (device layout -> reference layout), root row last."""
    X = H.uniform_corpus(300, dim, seed=17) * 1.1
    oix = H.oracle_index(X, storage, res, num_layers=2, ef_construction=16, ef_search=16)
    dix = H.device_index_from_oracle(oix, X)
    codes, mags = dix.download_codes()
    ocodes, omags = O.quantize_batch(np.vstack([X, oix.root_raw()[None, :]]), storage, res, -1.0, 1.0)
    assert np.array_equal(np.asarray(codes).reshape(301, -1), np.ascontiguousarray(ocodes).view(np.uint8).reshape(301, -1))
    assert np.array_equal(np.asarray(mags).view(np.uint32), omags.view(np.uint32))


# (name, cos_index_set_latency_mode, cos_index_set_latency_waves, cos_index_set_walk_order, level table on).  With a level table
# (u8 codes) the library picks the kernel itself (walk_kernel_kind), so the variants that name a kernel switch the table off.
WALK_VARIANTS = [("throughput kernel", 0, 0, 0, False), ("one-wave latency kernel where it applies", 0xFFFFFFFF, 0, 0, False),
                 ("four-wave latency kernel where it applies", 0xFFFFFFFF, 0xFFFFFFFF, 0, False),
                 ("throughput kernel, split walk in locality order", 0, 0, 1, False),
                 ("default policy with the level table (throughput kernel, or four waves above ef 64)", 0xFFFFFFFF, 0xFFFFFFFF, 0, True),
                 ("level table + split walk in locality order", 0, 0, 1, True)]


def _set_variant(dix, max_b, max_b4, order_min=0, table=False):
    import cosdata_amd as ca
    dix.set_latency_mode(max_b)
    dix.set_latency_waves(max_b4)
    dix.set_walk_order(order_min)
    dix.set_walk_table(ca.HNSWIndex.WALK_TABLE_AUTO if table else 0, 1 if table else 0)


def _reset_variant(dix):
    import cosdata_amd as ca
    dix.set_latency_mode(ca.HNSWIndex.LATENCY_MODE_DEFAULT_MAX_B)
    dix.set_latency_waves(ca.HNSWIndex.LATENCY_WAVES_DEFAULT_MAX_B)
    dix.set_walk_order(ca.HNSWIndex.WALK_ORDER_DEFAULT_MIN_B)
    dix.set_walk_table(ca.HNSWIndex.WALK_TABLE_AUTO, ca.HNSWIndex.WALK_TABLE_DEFAULT_MIN_B)


def _assert_same_search(oix, dix, Q, top_k):
    """every variant of the walk (cos_index_set_latency_mode / _waves: walk_kernel / walk_lat_kernel / walk_lat4_kernel) must give the oracle's answer"""
    oids, osc, ocnt = oix.search_batch(Q, top_k, threads=4)[:3]
    for vname, max_b, max_b4, order_min, table in WALK_VARIANTS:
        _set_variant(dix, max_b, max_b4, order_min, table)
        ids, sc, cnt = dix.batch_search(Q, top_k)
        assert np.array_equal(cnt, ocnt), vname
        for b in range(Q.shape[0]):
            c = int(cnt[b])
            assert np.array_equal(ids[b, :c], oids[b, :c]), f"{vname}: query {b}: ids differ\n{ids[b,:c]}\n{oids[b,:c]}"
            assert np.array_equal(sc[b, :c].view(np.uint32), osc[b, :c].view(np.uint32)), f"{vname}: query {b}: scores differ"
    _reset_variant(dix)


def ca_default_latency():
    import cosdata_amd as ca
    return ca.HNSWIndex.LATENCY_MODE_DEFAULT_MAX_B


def _assert_same_walk(oix, dix, Q):
    ow = [oix.ann_search(Q[b]) for b in range(Q.shape[0])]
    for vname, max_b, max_b4, order_min, table in WALK_VARIANTS:
        _set_variant(dix, max_b, max_b4, order_min, table)
        ids, sims, counts = dix.ann_search_batch(Q)
        for b in range(Q.shape[0]):
            oi, osim, olc = ow[b]
            assert np.array_equal(counts[b], olc), f"{vname}: query {b}: level counts {counts[b]} vs {olc}"
            off = 0
            for s, c in enumerate(olc):
                c = int(c)
                assert np.array_equal(ids[b, s, :c], oi[off:off + c]), f"{vname}: query {b} slot {s}: walk ids differ"
                assert np.array_equal(sims[b, s, :c].view(np.uint32), osim[off:off + c].view(np.uint32)), f"{vname}: query {b} slot {s}: sims differ"
                off += c
    _reset_variant(dix)


@pytest.mark.parametrize("name,storage,res", STORAGES)
@pytest.mark.parametrize("n,dim,ef", [(2000, 96, 64), (3000, 100, 32), (6000, 768, 256), (1000, 48, 32), (1500, 400, 40), (800, 16, 16),
                                      (1200, 1536, 64)])
def test_search_matches_oracle(name, storage, res, n, dim, ef):
    X = H.uniform_corpus(n, dim, seed=7)
    oix = H.oracle_index(X, storage, res, num_layers=5, ef_construction=64, ef_search=ef)
    dix = H.device_index_from_oracle(oix, X)
    Q = np.concatenate([H.queries_from(X, 24, seed=3), H.uniform_corpus(8, dim, seed=99)])
    _assert_same_walk(oix, dix, Q)
    _assert_same_search(oix, dix, Q, 10)
    _assert_same_search(oix, dix, Q, 5)


def test_search_clustered_default_params():
    X = H.clustered_corpus(20000, 128, seed=5)
    oix = H.oracle_index(X, O.STORAGE_U8, 0, ef_construction=64)
    dix = H.device_index_from_oracle(oix, X)
    Q = H.queries_from(X, 64, seed=11)
    _assert_same_walk(oix, dix, Q)
    _assert_same_search(oix, dix, Q, 10)


def test_rows_wider_than_64_go_to_the_one_wave_latency_kernel():
    """neighbour rows of 128 slots: walk_lat4_applicable must decline (its claim table is sized for rows of <= 64) and
    walk_lat_applicable accept.  Which kernel ran is read off the round count: the knob walk_lat_la = 1 narrows the window of the
    one-wave kernel alone to one entry, so that kernel, and no other, then issues exactly one round per expansion."""
    from cosdata_amd import _lib
    X = H.uniform_corpus(600, 48, seed=7)
    Q = np.concatenate([H.queries_from(X, 24, seed=3), H.uniform_corpus(8, 48, seed=99)])

    def rounds_per_variant(oix):
        dix = H.device_index_from_oracle(oix, X)
        _assert_same_walk(oix, dix, Q)
        out = {}
        with _lib.tuning(walk_lat_la=1):
            for vname, max_b, max_b4, order_min, table in WALK_VARIANTS[:3]:
                _set_variant(dix, max_b, max_b4, order_min, table)
                dix.batch_search(Q, 10)
                st = dix.last_stats()
                out[vname] = (int(st.reserved), int(st.expansions))
        _reset_variant(dix)
        return out

    wide = rounds_per_variant(H.oracle_index(X, O.STORAGE_U8, 0, num_layers=5, ef_construction=64, ef_search=32,
                                             neighbors_count=128, level0_neighbors_count=128))
    narrow = rounds_per_variant(H.oracle_index(X, O.STORAGE_U8, 0, num_layers=5, ef_construction=64, ef_search=32))
    tk, lat, lat4 = (v[0] for v in WALK_VARIANTS[:3])
    for r in (wide, narrow):
        assert r[tk][0] < r[tk][1], r          # the throughput kernel pops several window entries per round
        assert r[lat][0] == r[lat][1], r       # the one-wave kernel under the knob: one
    assert narrow[lat4][0] < narrow[lat4][1], narrow   # rows of <= 64: the four-wave kernel takes the launch
    assert wide[lat4] == wide[lat], wide               # rows of 128: it declines, the one-wave kernel runs


def test_zero_norm_query_is_calculation_error():
    import cosdata_amd as ca
    X = H.uniform_corpus(500, 96, seed=2)
    oix = H.oracle_index(X, O.STORAGE_U8, 0, num_layers=3, ef_construction=32, ef_search=32)
    dix = H.device_index_from_oracle(oix, X)
    Q = H.queries_from(X, 4)
    Q[2, :] = -1.0  # quantizes to all-zero bytes -> |q| = 0 -> DistanceError::CalculationError (cosine.rs:228-232)
    o = oix.search_batch(Q, 5, raise_on_error=False)
    for _, max_b, max_b4, order_min, table in WALK_VARIANTS:
        _set_variant(dix, max_b, max_b4, order_min, table)
        with pytest.raises(ca.CosdataError) as ei:
            dix.batch_search(Q, 5)
        assert ei.value.status == 2
        ids, sc, cnt, rc, status = dix.batch_search(Q, 5, return_status=True)
        assert rc == 2 and o[3] == 2
        assert np.array_equal(status, o[4])


@pytest.mark.parametrize("name,storage,res", STORAGES[:2])
def test_exact_visited_mode_matches_oracle(name, storage, res):
    """COS_VISITED_EXACT (recall mode): exact per-query visited bitset instead of the lossy PerformantFixedSet."""
    X = H.clustered_corpus(5000, 96, n_centers=16, seed=21)
    oix = H.oracle_index(X, storage, res, num_layers=4, ef_construction=48, ef_search=48)
    dix = H.device_index_from_oracle(oix, X)
    Q = H.queries_from(X, 40, seed=2)
    ref_ids = dix.batch_search(Q, 10)[0]
    oix.set_visited_mode(O.VISITED_EXACT)
    dix.set_visited_mode(1)
    _assert_same_walk(oix, dix, Q)
    _assert_same_search(oix, dix, Q, 10)
    exact_ids = dix.batch_search(Q, 10)[0]
    assert exact_ids.shape == ref_ids.shape


def test_auto_quantization_sampler_matches_oracle():
    import cosdata_amd as ca
    r = np.random.default_rng(4)
    for scale, n, d in [(0.036, 1000, 768), (0.2, 100, 96), (1.0, 64, 100), (0.01, 7, 33)]:
        x = (r.standard_normal((n, d)) * scale).astype(np.float32)
        assert ca.sample_values_range(x, 1.0) == O.sample_values_range(x, 1.0)
        assert ca.sample_values_range(x, 5.0) == O.sample_values_range(x, 5.0)


def _sampler_edge_inputs():
    """(name, sample [rows][dim], margin, expected range or None) that Gaussian draws never give.  The expectations state the rule
    (strict comparisons, `<=` on the tail share, -1 / 1 when no threshold holds); None = only the oracle says"""
    F = np.float32
    T = [F(t) for t in (0.025, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5)]
    up = T[1:] + [F(1.0)]
    cases = []
    for i, t in enumerate(T):                                    # 11 of 1000 values (1.1 %) on, just above and just below a threshold
        for what, v, want in (("on", t, t), ("above", np.nextafter(t, F(1)), up[i]), ("below", np.nextafter(t, F(0)), t)):
            x = np.zeros(1000, F)
            x[::97][:11] = v
            cases.append((f"{what} {t}", x.reshape(10, 100), 1.0, (-0.025, float(want))))
            cases.append((f"{what} -{t}", -x.reshape(10, 100), 1.0, (-float(want), 0.025)))
    x = np.zeros(1000, F)
    x[:10], x[500:510] = 0.7, -0.7                               # a tail share of exactly clamp_margin_percent: 10 of 1000, `<=` holds
    cases.append(("share on the margin", x.reshape(4, 250), 1.0, (-0.025, 0.025)))
    x = np.zeros(1000, F)
    x[:11], x[500:510] = 0.7, -0.7                               # ... and one value more above
    cases.append(("share above the margin", x.reshape(4, 250), 1.0, (-0.025, 1.0)))
    x = np.zeros(1000, F)
    x[:20], x[20:40], x[40:60] = np.nan, np.inf, -np.inf         # NaN is neither above nor below; the infinities are both tails' members
    cases.append(("NaN and infinities", x.reshape(10, 100), 1.0, (-1.0, 1.0)))
    cases.append(("NaN alone", np.full((3, 7), np.nan, F), 1.0, (-0.025, 0.025)))
    r = np.random.default_rng(8)
    x = np.abs(r.standard_normal((200, 64))).astype(F) * F(0.15)
    x[::3] *= F(-0.1)                                            # skewed: a long positive tail, a short negative one
    cases.append(("skewed", x, 1.0, None))
    cases.append(("skewed, margin 5", x, 5.0, None))
    for total in (1, 255, 257, 2048 * 256 + 3):                  # one lane; a ragged last wave; a second wave; a grid-stride tail of three
        k = total // 100 + 1                                     # the tail's share exceeds 1 % by the LAST elements alone
        x = np.zeros(total, F)
        x[total - k:] = 0.06
        cases.append((f"{total} values", x.reshape(1, total), 1.0, (-0.025, 0.1)))
        cases.append((f"{total} values, last one zero", np.concatenate([x[:-1], [F(0)]]).reshape(total, 1), 1.0, (-0.025, 0.025)))
    return cases


def test_auto_quantization_sampler_edge_inputs_match_oracle():
    """values on the thresholds and their f32 neighbours, a tail share that lands on the margin, NaN and +-inf, a sample with
    lo != -hi, and element counts around a wave and past the grid (the last elements decide)"""
    import cosdata_amd as ca
    asym = 0
    for name, x, margin, want in _sampler_edge_inputs():
        o = O.sample_values_range(x, margin)
        if want is not None:
            assert o == tuple(float(np.float32(w)) for w in want), (name, o, want)
        assert ca.sample_values_range(x, margin) == o, (name, o)
        asym += o[0] != -o[1]
    assert asym > 20


ALL_STORAGES = [("u8", O.STORAGE_U8, 0), ("bin", O.STORAGE_SUBBYTE, 1), ("q2", O.STORAGE_SUBBYTE, 2), ("oct", O.STORAGE_SUBBYTE, 3),
                ("f16", O.STORAGE_F16, 0), ("f32", O.STORAGE_F32, 0)]


@pytest.mark.parametrize("name,storage,res", ALL_STORAGES)
@pytest.mark.parametrize("dim", [100, 768])
def test_operators_every_storage_and_metric(name, storage, res, dim):
    """QuantizationMetric::quantize + DistanceMetric::calculate for every Storage kind x metric, incl. the error arms
    (StorageMismatch / CalculationError / unimplemented!) — values bit-exact vs the oracle."""
    import cosdata_amd as ca
    r = np.random.default_rng(17)
    x = r.uniform(-1.2, 1.2, (40, dim)).astype(np.float32)
    x[3] = 0.0
    x[4] = -1.0
    stype = ca.StorageType(ca.StorageKind(storage), res)
    codes, mags = ca.ScalarQuantization.quantize(x, stype, (-1.0, 1.0))
    ocodes, omags = O.quantize_batch(x, storage, res, -1.0, 1.0)
    assert np.array_equal(codes, ocodes)
    assert np.array_equal(mags.view(np.uint32), omags.view(np.uint32))
    px = r.integers(0, 40, 96).astype(np.uint32)
    py = r.integers(0, 40, 96).astype(np.uint32)
    px[:2], py[:2] = [3, 4], [5, 6]
    for metric in (O.METRIC_COSINE, O.METRIC_EUCLIDEAN, O.METRIC_HAMMING, O.METRIC_DOT):
        vals, status = ca.distance_batch(ca.DistanceMetric(metric), stype, dim, codes, mags, codes, mags, px, py)
        for p in range(px.size):
            rc, v = O.distance(metric, storage, res, dim, ocodes[px[p]], omags[px[p]], ocodes[py[p]], omags[py[p]])
            assert status[p] == rc, (name, metric, p, status[p], rc)
            if rc == 0:
                assert np.float32(vals[p]).tobytes() == np.float32(v).tobytes() or (np.isnan(vals[p]) and np.isnan(v)), (name, metric, p, vals[p], v)
