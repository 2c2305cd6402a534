"""A small collection with a metadata schema, in the numeric form the engine takes.

Default schema (what metadata/schema.rs would encode): field `color` with values 1..3 (2 binary dims), field `size` with values 1..5
(3 dims), supported conditions AND(color, size) -> 5 metadata dimensions, max_replicas_per_node = 4:
    base id 4r        Base replica (all-zero dims: lives under the MAIN root, not in the pseudo-root component)
    4r + 1            color only      [c1 c0 | 0 0 0]
    4r + 2            size only       [0 0 | s2 s1 s0]
    4r + 3            color AND size  [c1 c0 | s2 s1 s0]
Pseudo nodes (api_service.rs:135-210): the pseudo root u32::MAX - 257 with all dims = HIGH_WEIGHT (1), then one node per
value combination (3 + 5 + 15), all sharing the all-zero vector.

Scenario takes any other schema as fields, conditions and max_replicas; MDIM and REPLICAS are the default's values."""
from __future__ import annotations

import itertools

import numpy as np

from oracle import oracle as O
from tests import helpers as H

PSEUDO_ROOT = 0xFFFFFFFF - 257
MDIM, REPLICAS = 5, 4


def bits(v: int, size: int):
    return [(v >> (size - 1 - i)) & 1 for i in range(size)]


def dims(color=None, size=None, neq_color=False, neq_size=False):
    """metadata / filter dimensions: Equal -> the binary digits, NotEqual -> 1 -> -1, 0 -> 1 (query_filtering.rs:29-45)"""
    enc = lambda b, neq: [(-1 if x else 1) for x in b] if neq else b
    c = enc(bits(color, 2), neq_color) if color is not None else [0, 0]
    s = enc(bits(size, 3), neq_size) if size is not None else [0, 0, 0]
    return c + s


DEFAULT_FIELDS = [(3, 2), (5, 3)]                       # (cardinality, binary dims): color, size
DEFAULT_CONDITIONS = [(0,), (1,), (0, 1)]               # supported AND-conditions as tuples of field indices

# the schemas of tests/test_gpu_meta_schemas.py and tests/test_oracle_pymeta.py: (fields, conditions, max_replicas)
#   A: 9 dims = one 8-chain pass of the metadata dot + a tail of 1, stride 5;  B: 16 dims = two passes, no tail, stride 6
#   C: the smallest schema there is (1 dim, stride 2);  D: 64 dims = the limit of cos_index_enable_metadata, stride 7
SCHEMAS = {
    "A": dict(fields=[(6, 3), (9, 4), (3, 2)], conditions=[(0,), (1,), (2,), (0, 1)], max_replicas=5),
    "B": dict(fields=[(5, 4), (6, 4), (15, 4), (3, 4)], conditions=[(0,), (1,), (2,), (3,), (0, 1)], max_replicas=6),
    "C": dict(fields=[(1, 1)], conditions=[(0,)], max_replicas=2),
    "D": dict(fields=[(3, 2)] * 2 + [(2, 10)] * 6, conditions=[(0,), (1,), (0, 1), (2,), (3,), (7,)], max_replicas=7),
}


class Scenario:
    """fields = [(cardinality, nbits)]: field f takes the values 1..cardinality, written in nbits binary dims; conditions = the
    supported AND-conditions (tuples of field indices): replica max_replicas * r + 1 + i of embedding r carries condition i, and
    every value combination of a condition has one pseudo node (root first, then condition by condition in product order)"""

    def __init__(self, n=1500, dim=64, seed=0, storage=O.STORAGE_U8, res=0, fields=None, conditions=None, max_replicas=REPLICAS,
                 metric=O.METRIC_COSINE, shortlist_size=64, **hp):
        rng = np.random.default_rng(seed)
        self.n, self.dim = n, dim
        self.fields = [tuple(f) for f in (DEFAULT_FIELDS if fields is None else fields)]
        self.conditions = [tuple(c) for c in (DEFAULT_CONDITIONS if conditions is None else conditions)]
        self.replicas = int(max_replicas)
        self.mdim = sum(nb for _, nb in self.fields)
        assert 1 <= len(self.conditions) < self.replicas and all(card < (1 << nb) for card, nb in self.fields)
        self.names = ["color", "size"] if self.fields == DEFAULT_FIELDS else [f"f{i}" for i in range(len(self.fields))]
        self.X = H.clustered_corpus(n, dim, n_centers=10, sigma=0.25, seed=seed + 1)
        self.values = [rng.integers(1, card + 1, n) for card, _ in self.fields]
        for name, v in zip(self.names, self.values):
            setattr(self, name, v)
        ids, mb = [], []
        for r in range(n):
            for i, cond in enumerate(self.conditions):
                ids.append(self.replicas * r + 1 + i)
                mb.append(self.dims({f: int(self.values[f][r]) for f in cond}))
        pseudo = [[1] * self.mdim]
        for cond in self.conditions:
            pseudo += [self.dims(dict(zip(cond, combo))) for combo in itertools.product(*[range(1, self.fields[f][0] + 1) for f in cond])]
        ids += [PSEUDO_ROOT + i for i in range(len(pseudo))]
        mb += pseudo
        self.node_ids = np.array(ids, np.uint32)
        self.mbits = np.array(mb, np.int32)
        # enough slots for the root to keep an edge to every pseudo node and enough layers for the top mixed level to hold only
        # a handful of replicas: a matching pseudo node whose slots fill up with replicas EVICTS its edge to the root
        # (prob_node.rs:271-279), after which a filtered walk can only enter it from above
        self.hp = dict(num_layers=6, ef_construction=48, ef_search=64, neighbors_count=32, level0_neighbors_count=64)
        self.hp.update(hp)
        L = self.hp["num_layers"]
        # level draws as the reference makes them: replicas from the schema-adjusted levels_prob (api_service.rs:113-131: the
        # upper layers belong to the pseudo nodes), pseudo nodes from pseudo_level_probs over the non-root pseudo nodes
        lp, plp = O.schema_level_probs(L, len(pseudo)), O.pseudo_level_probs(L, len(pseudo) - 1)
        self.max_levels = np.array([O.max_insert_level(float(np.float32(rng.random())), plp if i >= PSEUDO_ROOT else lp)
                                    for i in self.node_ids], np.uint8)
        self.params = O.HNSWParams(dim=dim, storage=storage, resolution=res, seed=seed + 5, metric=metric, shortlist_size=shortlist_size,
                                   **self.hp)
        # which condition an "is" / "and" query kind asks for, and the two conditions of an "or" query (see queries())
        multi = [i for i, c in enumerate(self.conditions) if len(c) > 1]
        self.kind_cond = {}
        for i, cond in enumerate(self.conditions):
            name = "is_" + self.names[cond[0]] if len(cond) == 1 else "and" if len(multi) == 1 else "and_" + "_".join(map(str, cond))
            self.kind_cond[name] = i
        self.or_conds = (0, min(1, len(self.conditions) - 1))

    def dims(self, eq, neq=()):
        """metadata / filter dimensions of {field: value}: Equal -> the binary digits, NotEqual (fields in `neq`) -> 1 -> -1, 0 -> 1
        (query_filtering.rs:29-45); fields that are not named stay 0"""
        out = []
        for f, (card, nb) in enumerate(self.fields):
            if f not in eq:
                out += [0] * nb
                continue
            b = bits(min(int(eq[f]), card), nb)          # a value beyond the cardinality could encode as all zeros
            out += [(-1 if x else 1) for x in b] if f in neq else b
        return out

    def oracle(self):
        oix = O.OracleIndex(self.params).set_vectors(self.X)
        oix.meta_enable(self.mdim, self.replicas)          # before any graph: base ids become max_replicas * r
        oix.build()
        oix.meta_set_nodes(self.node_ids, self.mbits).meta_build(self.max_levels)
        return oix

    def device_index(self, id_base=0):
        """an empty device handle with this scenario's parameters, vectors and schema"""
        import cosdata_amd as ca
        p = self.params
        hp = ca.HNSWHyperParams(num_layers=p.num_layers, ef_construction=p.ef_construction, ef_search=p.ef_search,
                                level_0_neighbors_count=p.level0_neighbors_count, neighbors_count=p.neighbors_count)
        dix = ca.HNSWIndex(self.dim, hp, ca.DistanceMetric(p.metric), ca.StorageType(ca.StorageKind(p.storage), p.resolution),
                           (p.range_lo, p.range_hi), p.shortlist_size, id_base=id_base)
        dix.upload_vectors(self.X).enable_metadata(self.mdim, self.replicas)
        return dix

    def device(self, oix, id_base=0):
        dix = self.device_index(id_base)
        dix.upload_graph(oix.export_graph(), oix.root_raw())
        dix.upload_meta_graph(self.node_ids, self.mbits, oix.meta_export_graph())
        return dix

    def queries(self, nq=24, seed=3):
        """(Q, offsets, filter rows, description per query).  The kinds cycle: "is" on every supported condition in turn (the
        multi-field one is "and"), OR of two conditions, NotEqual on one field, and a mix of three filters.  A description is
        (kind, value of field 0, value of field 1, ...) with None for the fields the query does not name.  No filter row is all
        zero: that would be a Base-kind query under the pseudo root."""
        rng = np.random.default_rng(seed)
        Q = H.queries_from(self.X, nq, noise=0.05, seed=seed)
        nc = len(self.conditions)
        wide = max(self.conditions, key=len)              # the first of the widest conditions
        f0 = self.conditions[0][0]
        off, rows, desc = [0], [], []
        for b in range(nq):
            v = [int(rng.integers(1, card + 1)) for card, _ in self.fields]
            cond = lambda i: {f: v[f] for f in self.conditions[i]}
            other = dict(cond(0))
            other[f0] = (v[f0] % self.fields[f0][0]) + 1  # another value of the first field (the same one at cardinality 1)
            kind = b % (nc + 3)
            if kind < nc:
                f, name = [cond(kind)], [k for k, i in self.kind_cond.items() if i == kind][0]
            elif kind == nc:
                f, name = [cond(0), cond(self.or_conds[1]) if nc > 1 else other], "or"
            elif kind == nc + 1:
                f, name = [{f0: v[f0]}], "neq_" + self.names[f0]
            else:
                f, name = [{g: v[g] for g in wide}, cond(self.or_conds[1]), other], "mixed"
            neq = [(f0,)] if kind == nc + 1 else [(wide[-1],), (), ()] if kind == nc + 2 else [()] * len(f)
            named = set().union(*f)
            rows += [self.dims(e, q) for e, q in zip(f, neq)]
            off.append(len(rows))
            desc.append((name,) + tuple(v[g] if g in named else None for g in range(len(self.fields))))
        rows = np.array(rows, np.int32)
        assert rows.any(axis=1).all()
        return Q, np.array(off, np.uint32), rows, desc
