"""What the device tests of tests/test_gpu_meta_append.py rest on, checked without a device: every split they use ends the old build
on a batch boundary of the whole build (tests/meta_append.py), and the oracle's base graph of a metadata collection continues."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import meta_append as MA
from tests import meta_helpers as MH


@pytest.mark.parametrize("name", sorted(MA.CASES))
def test_every_split_of_the_device_tests_is_admissible(name):
    sc, sp, batch, _ = MA.case(name)                        # (Split asserts it)
    assert sp.batch == (batch or 1024)
    new = sum(int(m.sum()) for m in sp.steps)
    assert int(sp.old.sum()) + new == sc.node_ids.size and new > 0
    assert sp.inserted_at[0] == MA.inserted_nodes(*sp.table(sp.old)[:2])


def test_the_issue_s_splits_and_a_split_that_is_not_admissible():
    sc = MH.Scenario(n=MA.N, dim=32, seed=2)
    sp = MA.Split(sc, (302, 310, MA.N), 8)
    assert sp.inserted_at == [23 + 3 * 302, 23 + 3 * 310]    # 23 non-root pseudo nodes, 3 Metadata replicas per embedding
    assert [int(m.sum()) for m in sp.steps] == [24, 870]
    assert (sp.table(sp.steps[0])[2] > 0).any() or (sp.table(sp.steps[1])[2] > 0).any()
    MA.Split(sc, (456, MA.N), 0)                             # the default batch, never capped at this size
    with pytest.raises(AssertionError, match="not admissible"):
        MA.Split(sc, (303, MA.N), 8)
    for n0 in (1, 17, 417, 599):                             # batches of one: the sequential reference order, every cut
        MA.Split(sc, (n0, MA.N), 1)
    assert MA.boundaries(20, 8)[:12] == [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 15]


def test_oracle_base_graph_of_a_metadata_collection_continues():
    """build_rounds(b) on X[:n0] + append(X[n0:], b) == build_rounds(b) on X for n0 on a boundary of the BASE schedule; ids = row x replicas"""
    sc = MH.Scenario(n=400, dim=32, seed=6)
    b, n0 = 16, 254
    assert n0 in MA.boundaries(sc.n, b)
    whole = O.OracleIndex(sc.params).set_vectors(sc.X)
    whole.meta_enable(sc.mdim, sc.replicas)
    whole.build_rounds(b, greedy=False)
    part = O.OracleIndex(sc.params).set_vectors(sc.X[:n0])
    part.meta_enable(sc.mdim, sc.replicas)
    part.build_rounds(b, greedy=False)
    part.append(sc.X[n0:], b)
    for l, ((pi, pn), (wi, wn)) in enumerate(zip(part.export_graph(), whole.export_graph())):
        assert np.array_equal(pi, wi) and np.array_equal(pn, wn), f"level {l}"
        real = pi[pi != 0xFFFFFFFF]
        assert (real % sc.replicas == 0).all() and (l > 0 or real.size == sc.n)
