"""The builder's walks under cos_index_set_latency_mode over f32 / f16 rows and binary / octal codes (indexing mode: keep 64, own id
seeded in the filter): the device build equals the oracle's build_rounds slot for slot, and the built graph answers like the oracle."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests.test_gpu_builder import _assert_same_graph, _device_index

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("waves", [0, 2048])
@pytest.mark.parametrize("storage,res", [(O.STORAGE_F32, 0), (O.STORAGE_F16, 0), (O.STORAGE_SUBBYTE, 1), (O.STORAGE_SUBBYTE, 3)])
def test_device_build_on_the_latency_kernels_equals_oracle_rounds(storage, res, waves):
    dim, bs = 128, 512
    X = H.clustered_corpus(4000, dim, n_centers=16, seed=9)
    kw = dict(num_layers=5, ef_construction=64, ef_search=64, seed=77)
    dix = _device_index(X, storage, res, latency=2048, waves=waves, **kw).build(bs)
    oix = O.OracleIndex(O.HNSWParams(dim=dim, storage=storage, resolution=res, **kw)).set_vectors(X).build_rounds(bs, greedy=False)[0]
    _assert_same_graph(dix, oix)
    Q = H.queries_from(X, 32, seed=5)
    ids, sc, cnt = dix.batch_search(Q, 10)
    assert dix.last_walk_kernel() == ("latency_waves" if waves else "latency")
    oids, osc, ocnt = oix.search_batch(Q, 10, threads=4)[:3]
    assert np.array_equal(ids, oids) and np.array_equal(sc.view(np.uint32), osc.view(np.uint32)) and np.array_equal(cnt, ocnt)
