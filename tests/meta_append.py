"""Appending embeddings to a collection with a metadata schema (cos_index_append + cos_index_append_meta): a meta_helpers.Scenario of n
embeddings cut at n0 — the node table of the first n0 embeddings (replica ids below n0 x replicas, plus every pseudo node) is what the
old build saw, the rest is what the append adds.

The statement the device is held to is ONE oracle meta_build_rounds over the whole table.  That holds when T0, the number of nodes the
old build inserted (pseudo nodes without the pseudo root + Metadata replicas), is a boundary of the unclamped schedule
inserted += min(B, max(1, inserted // 4)): the old build's last batch then ends where a batch of the full build ends.  Split asserts it,
so that a split that is not admissible fails as such and not as "graphs differ"."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from tests import meta_helpers as MH

DEFAULT_BATCH = 1024          # cos_index_build_meta / cos_index_append_meta with batch_size = 0


def boundaries(upto: int, batch: int):
    """every value `inserted` takes in the unclamped schedule, up to `upto`"""
    out, at = [0], 0
    while at < upto:
        at += min(batch, max(1, at // 4))
        out.append(at)
    return out


def inserted_nodes(node_ids, mbits) -> int:
    """nodes a build of this table inserts: all but the pseudo root and the Base replicas (all-zero metadata dimensions)"""
    ids, mb = np.asarray(node_ids), np.asarray(mbits)
    return int(((ids != MH.PSEUDO_ROOT) & mb.any(axis=1)).sum())


def device_base(sc: MH.Scenario, n0: int, base_batch: int):
    """the first n0 vectors of `sc` on a handle with the schema enabled and the base graph built on the device (the oracle's seed)"""
    import cosdata_amd as ca
    p = sc.params
    hp = ca.HNSWHyperParams(num_layers=p.num_layers, ef_construction=p.ef_construction, ef_search=p.ef_search,
                            level_0_neighbors_count=p.level0_neighbors_count, neighbors_count=p.neighbors_count)
    dix = ca.HNSWIndex(sc.dim, hp, ca.DistanceMetric(p.metric), ca.StorageType(ca.StorageKind(p.storage), p.resolution),
                       (p.range_lo, p.range_hi), p.shortlist_size, seed=p.seed)
    dix.upload_vectors(sc.X[:n0]).enable_metadata(sc.mdim, sc.replicas)
    return dix.build(base_batch)


class Split:
    """the node table of `sc` cut into the first n0 embeddings (+ every pseudo node) and the rest, optionally in several steps:
    cuts = (n0, n1, ..., n) -> one old table and len(cuts) - 1 appends"""

    def __init__(self, sc: MH.Scenario, cuts, batch: int, node_ids=None, mbits=None, max_levels=None):
        self.sc, self.cuts, self.batch = sc, tuple(cuts), batch or DEFAULT_BATCH
        self.node_ids = sc.node_ids if node_ids is None else node_ids
        self.mbits = sc.mbits if mbits is None else mbits
        self.max_levels = sc.max_levels if max_levels is None else max_levels
        assert (np.diff(self.node_ids.astype(np.int64)) > 0).all() and self.cuts[-1] == sc.n and list(self.cuts) == sorted(set(self.cuts))
        pseudo = self.node_ids >= MH.PSEUDO_ROOT
        emb = self.node_ids // sc.replicas
        self.old = pseudo | (emb < self.cuts[0])
        self.steps = [~pseudo & (emb >= a) & (emb < b) for a, b in zip(self.cuts[:-1], self.cuts[1:])]
        # admissible: every call but the last ends on a batch boundary of the whole build
        bounds = set(boundaries(inserted_nodes(self.node_ids, self.mbits), self.batch))
        at = inserted_nodes(self.node_ids[self.old], self.mbits[self.old])
        self.inserted_at = [at]
        for m in self.steps[:-1]:
            at += inserted_nodes(self.node_ids[m], self.mbits[m])
            self.inserted_at.append(at)
        for t in self.inserted_at:
            assert t in bounds, f"{t} inserted nodes is no boundary of the schedule at batch {self.batch}: the split {self.cuts} is not admissible"

    def table(self, mask):
        return self.node_ids[mask], self.mbits[mask], self.max_levels[mask]

    # ---- the oracle's side --------------------------------------------------------------------------------------------------
    def oracle_base(self, base_batch):
        """the base graph as the device makes it: build_rounds on the first n0 vectors, then one append per step"""
        sc = self.sc
        oix = O.OracleIndex(sc.params).set_vectors(sc.X[:self.cuts[0]])
        oix.meta_enable(sc.mdim, sc.replicas)
        oix.build_rounds(base_batch, greedy=False)
        for a, b in zip(self.cuts[:-1], self.cuts[1:]):
            oix.append(sc.X[a:b], base_batch)
        return oix

    def oracle_whole(self, base_batch):
        """base graph as above; the component: ONE meta_build_rounds over the whole table"""
        oix = self.oracle_base(base_batch)
        oix.meta_set_nodes(self.node_ids, self.mbits).meta_build_rounds(self.max_levels, self.batch)
        return oix

    # ---- the device's side --------------------------------------------------------------------------------------------------
    def device_old(self, base_batch):
        """a handle with the first n0 vectors, the schema, the base graph and the old table's component, all built on the device"""
        dix = device_base(self.sc, self.cuts[0], base_batch)
        dix.build_meta(*self.table(self.old), self.batch)
        return dix

    def device_step(self, dix, step, base_batch, batch_arg=None):
        a, b = self.cuts[step], self.cuts[step + 1]
        dix.append(self.sc.X[a:b], base_batch)
        dix.append_meta(*self.table(self.steps[step]), self.batch if batch_arg is None else batch_arg)
        return dix


# the cases of tests/test_gpu_meta_append.py: name -> (Scenario arguments, component batch as given to the device, cuts, base-graph batch)
N = 600
CASES = {
    "default-b8": (dict(dim=64, seed=21), 8, (302, N), 8),
    "default-b0": (dict(dim=64, seed=22), 0, (456, N), 64),
    "schemaD-b8": (dict(dim=64, seed=23, **MH.SCHEMAS["D"]), 8, (302, N), 16),
    "schemaC-q2-b48": (dict(dim=128, seed=24, storage=O.STORAGE_SUBBYTE, res=2, **MH.SCHEMAS["C"]), 48, (330, N), 48),
    "schemaA-f16-b1": (dict(dim=72, seed=25, storage=O.STORAGE_F16, **MH.SCHEMAS["A"]), 1, (417, N), 64),
    "default-b8-twice": (dict(dim=64, seed=26), 8, (302, 310, N), 8),
}


def case(name):
    """(Scenario, Split, batch argument for the device, base-graph batch)"""
    kw, batch, cuts, base_batch = CASES[name]
    sc = MH.Scenario(n=N, **kw)
    return sc, Split(sc, cuts, batch), batch, base_batch


def assert_same_levels(got, want, what=""):
    assert len(got) == len(want)
    for l, ((gi, gn), (ei, en)) in enumerate(zip(got, want)):
        assert np.array_equal(gi, ei), f"{what}level {l}: node sets differ ({len(gi)} vs {len(ei)} nodes)"
        assert np.array_equal(gn, en), f"{what}level {l}: adjacency differs in {np.count_nonzero((gn != en).any(axis=1))} of {len(en)} rows"
