"""Shared by test_mutation_scenario.py (CPU) and test_gpu_mutation_coherence.py (GPU): one history of appends and deletes on a small
dense index, stated on the CPU oracle alone — the corpus, the hyper-parameters, the steps, the ids the deletes take (chosen by level
membership, so that they touch what the level table and the locality order cover) and the queries.  The GPU tests replay the steps on
a handle whose caches are warm and compare every search path with a handle that never saw another graph and with the oracle; the CPU
test checks that the history moves the answers at all, without which a stale cache would go unnoticed."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

from oracle import oracle as O
from tests import helpers as H

N0, BATCH = 3000, 256
FULL_HISTORY = (("append", 1), ("append", 700), ("append", 800), ("delete", 1), ("delete", 39), ("delete", 120), ("append", 300))
SHORT_HISTORY = (("append", 700), ("delete", 40), ("append", 300))
ROOT = 0xFFFFFFFF


def scale_of(storage):
    return 0.9 if storage == O.STORAGE_SUBBYTE else 1.0      # SubByte levels are hard-wired to [-1, 1): keep the corpus inside


@dataclass
class Scenario:
    params: O.HNSWParams
    X: np.ndarray                      # every vector the history ever holds, in id order
    history: Tuple[Tuple[str, int], ...]
    steps: List[Tuple[str, object]]    # ("append", (first, last)) rows of X | ("delete", ids u32[])
    victims: np.ndarray                # every deleted id, in the order of deletion
    victim_levels: np.ndarray          # the highest level of each of them when it was chosen
    Q: np.ndarray                      # 4096 queries near the vectors resident when the victims are chosen; tests use prefixes
    Qv: np.ndarray                     # as many queries as victims, each near one of them (drawn with replacement)
    n_at: List[int] = field(default_factory=list)   # resident vectors at every point of the history (point 0 = before the first step)

    def oracle(self):
        """a fresh oracle index at point 0 of the history"""
        oix = O.OracleIndex(self.params).set_vectors(self.X[:N0])
        oix.build_rounds(BATCH)
        return oix

    def apply(self, ix, step):
        """step `step` (0-based) on an oracle index or a device handle that owns its rows: both spell append / delete alike"""
        kind, what = self.steps[step]
        if kind == "append":
            ix.append(self.X[what[0]:what[1]], BATCH)
        else:
            ix.delete(what)


def level_sets(graph):
    """per level: the vector ids of its nodes (the root left out)"""
    return [set(int(i) for i in ids if i != ROOT) for ids, _ in graph]


def level_counts(oix):
    return [len(ids) for ids, _ in oix.export_graph()]


def _pick_victims(graph, n_victims, rng):
    """n / 20 ids of the top level, 3n / 20 whose highest level is the one below, 6n / 20 one further down, the other half on level 0
    only (160 -> 8, 24, 48, 80), shuffled"""
    sets = level_sets(graph)
    top = len(sets) - 1
    assert top == 3
    only = {top: sets[top]}
    for l in range(top - 1, -1, -1):
        only[l] = sets[l] - sets[l + 1]
    want = {3: n_victims // 20, 2: 3 * n_victims // 20, 1: 6 * n_victims // 20}
    want[0] = n_victims - sum(want.values())
    ids, lv = [], []
    for l in (3, 2, 1, 0):
        pool = np.array(sorted(only[l]), np.uint32)
        assert pool.size >= want[l], (l, pool.size, want[l])
        take = rng.choice(pool, size=want[l], replace=False)
        ids.append(take)
        lv.append(np.full(want[l], l, np.int32))
    ids, lv = np.concatenate(ids).astype(np.uint32), np.concatenate(lv)
    perm = rng.permutation(ids.size)
    return ids[perm], lv[perm]


def make(history=FULL_HISTORY, dim=96, storage=O.STORAGE_U8, resolution=0) -> Scenario:
    """the shape of tests/test_gpu_walk_plan.py (its thresholds are crossed with few queries): 3 layers, M 16 / 32, ef 32, seed 5,
    build(256) of 3000 clustered vectors; the victims of ALL deletes are chosen once, in the oracle's graph in front of the first delete"""
    total = N0 + sum(m for k, m in history if k == "append")
    X = H.clustered_corpus(total, dim, n_centers=16, seed=11) * np.float32(scale_of(storage))
    p = O.HNSWParams(dim=dim, storage=storage, resolution=resolution, num_layers=3, ef_construction=32, ef_search=32,
                     level0_neighbors_count=32, neighbors_count=16, seed=5)
    sc = Scenario(p, X, tuple(history), [], np.zeros(0, np.uint32), np.zeros(0, np.int32), X[:0], X[:0])
    oix = sc.oracle()
    at, n_at, chunks, steps = N0, [N0], None, []
    n_victims = sum(m for k, m in history if k == "delete")
    for kind, m in history:
        if kind == "append":
            steps.append(("append", (at, at + m)))
            oix.append(X[at:at + m], BATCH)
            at += m
        else:
            if chunks is None:                      # the first delete: the graph as it is now decides who goes, for every delete
                sc.victims, sc.victim_levels = _pick_victims(oix.export_graph(), n_victims, np.random.default_rng(5))
                sc.Q = H.queries_from(X[:at], 4096, noise=0.05, seed=3)
                sc.Qv = H.queries_from(X[sc.victims], n_victims, noise=0.05, seed=9)
                chunks = 0
            ids = sc.victims[chunks:chunks + m]
            chunks += m
            steps.append(("delete", ids))
            oix.delete(ids)
        n_at.append(at)
    assert chunks == n_victims
    sc.steps, sc.n_at = steps, n_at
    return sc


def changed_share(before, after):
    """share of the queries whose (ids, score bits, counts) differ between two search_batch results"""
    (ia, sa, ca), (ib, sb, cb) = before[:3], after[:3]
    same = (ia == ib).all(axis=1) & (sa.view(np.uint32) == sb.view(np.uint32)).all(axis=1) & (ca == cb)
    return 1.0 - float(same.mean())
