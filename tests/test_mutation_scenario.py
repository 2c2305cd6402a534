"""CPU: the conditions that make tests/test_gpu_mutation_coherence.py sensitive, on the oracle alone.  A cache that went stale would
return the PREVIOUS graph's answer, which only shows where the answers move: every big step of tests/mutation_scenario.py must change
the (ids, score bits) of a large share of the queries, the levels the table and the order cover must grow, and the deletes must take
nodes of every level."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import mutation_scenario as M


@pytest.fixture(scope="module")
def full():
    return M.make()


def _walk_history(sc, queries):
    """[(level counts, {name: search_batch result})] at every point of the history"""
    oix = sc.oracle()
    points = []
    for point in range(len(sc.steps) + 1):
        if point:
            sc.apply(oix, point - 1)
        points.append((M.level_counts(oix), {k: oix.search_batch(q, 10, threads=4) for k, q in queries.items()}))
    return points


def test_the_scenario_is_the_one_the_gpu_tests_assume(full):
    sc = full
    assert sc.history == M.FULL_HISTORY and len(sc.steps) == 7
    assert sc.n_at == [3000, 3001, 3701, 4501, 4501, 4501, 4501, 4801] and sc.X.shape == (4801, 96)
    assert [s[0] for s in sc.steps] == ["append"] * 3 + ["delete"] * 3 + ["append"]
    assert [s[1].size for s in sc.steps[3:6]] == [1, 39, 120]
    assert np.array_equal(np.concatenate([s[1] for s in sc.steps[3:6]]), sc.victims)
    assert np.unique(sc.victims).size == 160 and sc.victims.max() < 4501
    assert sc.Q.shape == (4096, 96) and sc.Qv.shape == (160, 96)


def test_the_victims_come_from_every_level(full):
    """8 ids of level 3, 24 whose highest level is 2, 48 whose highest level is 1, 80 on level 0 only — checked against the oracle's
    graph in front of the first delete, not against the picker's own bookkeeping"""
    sc = full
    oix = sc.oracle()
    for step in range(3):
        sc.apply(oix, step)
    sets = M.level_sets(oix.export_graph())
    top = [max(l for l in range(4) if int(v) in sets[l]) for v in sc.victims]
    assert np.bincount(top, minlength=4).tolist() == [80, 48, 24, 8]
    assert np.array_equal(np.array(top), sc.victim_levels)
    # ... so that every delete chunk but the single id reaches the levels the table (levels 1-3) and the order key (level 1) cover
    assert (sc.victim_levels[1:40] >= 1).any() and (sc.victim_levels[40:] >= 1).sum() >= 40


def test_every_big_step_moves_the_answers(full):
    """Share of the queries whose (ids, score bits, counts) change over a step, measured on the oracle (Q[:512] / Qv):
        append 1     0.002 / 0.000      delete 1     0.000 / 0.031
        append 700   0.867 / 0.856      delete 39    0.074 / 0.275
        append 800   0.863 / 0.900      delete 120   0.217 / 0.819
                                        append 300   0.502 / 0.531
    The floors are half of what was measured (0.87, 0.87, 0.81 of Qv, 0.50): a changed seed in a helper does not break them by a hair,
    a history that stopped mattering does.  Level sizes: 3001/731/194/42 -> 3002/731/194/42 -> 3702/942/246/54 -> 4502/1133/295/64
    -> (deletes keep them) -> 4802/1212/314/69."""
    sc = full
    pts = _walk_history(sc, {"Q": sc.Q[:512], "Qv": sc.Qv})
    share = lambda step, k: M.changed_share(pts[step][1][k], pts[step + 1][1][k])     # step: 0-based index into sc.steps
    assert share(1, "Q") >= 0.4, share(1, "Q")            # append 700
    assert share(2, "Q") >= 0.4, share(2, "Q")            # append 800
    assert share(5, "Qv") >= 0.4, share(5, "Qv")          # delete 120
    assert share(6, "Q") >= 0.25, share(6, "Q")           # append 300 after the deletes
    counts = [c for c, _ in pts]
    assert [c[0] for c in counts] == [n + 1 for n in sc.n_at]
    for step in (1, 2, 6):                                # the table levels (1-3) grow at the three big appends: more columns, a wider stride
        assert sum(counts[step + 1][1:]) > sum(counts[step][1:]), (step, counts[step], counts[step + 1])
        assert counts[step + 1][1] > counts[step][1]      # ... and so does the order's key level
    for step in (3, 4, 5):                                # a delete unlinks, it removes no node
        assert counts[step + 1] == counts[step]
    # the table's stride (columns rounded up to 32) and the exact filter's words per query (largest level / 32) really change
    stride = lambda c: (sum(c[1:]) + 31) // 32 * 32
    assert stride(counts[2]) > stride(counts[1]) and stride(counts[3]) > stride(counts[2]) and stride(counts[7]) > stride(counts[6])
    assert (counts[7][0] + 31) // 32 > (counts[3][0] + 31) // 32 > (counts[0][0] + 31) // 32


@pytest.mark.parametrize("name,kw", [("short", {}), ("q2", dict(dim=128, storage=O.STORAGE_SUBBYTE, resolution=2)), ("f16", dict(storage=O.STORAGE_F16))])
def test_the_short_history_moves_the_answers_too(name, kw):
    """append 700, delete 40, append 300.  Measured shares (Q[:512] / Qv):
        u8 x 96      1.000 / 1.000   0.115 / 0.250   0.953 / 0.950
        q2 x 128     0.771 / 0.775   0.133 / 0.400   0.871 / 0.875
        f16 x 96     0.869 / 0.850   0.127 / 1.000   0.533 / 0.550
    floors = half of the smallest measured value of a column: 0.38 for the first append, 0.12 of Qv for the delete, 0.26 for the last append"""
    sc = M.make(M.SHORT_HISTORY, **kw)
    assert sc.n_at == [3000, 3700, 3700, 4000] and np.bincount(sc.victim_levels).tolist() == [20, 12, 6, 2]
    pts = _walk_history(sc, {"Q": sc.Q[:512], "Qv": sc.Qv})
    share = lambda step, k: M.changed_share(pts[step][1][k], pts[step + 1][1][k])
    assert share(0, "Q") >= 0.38 and share(1, "Qv") >= 0.12 and share(2, "Q") >= 0.26, [share(s, k) for s in range(3) for k in ("Q", "Qv")]
    counts = [c for c, _ in pts]
    assert sum(counts[1][1:]) > sum(counts[0][1:]) and counts[2] == counts[1] and sum(counts[3][1:]) > sum(counts[2][1:])
