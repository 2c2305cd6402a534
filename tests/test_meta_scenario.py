"""tests/meta_helpers.Scenario takes any schema; its default must stay the collection every earlier metadata test was written
against, bit for bit: the digests below were taken from the two-field Scenario before it learned about other schemas."""
import hashlib

import numpy as np
import pytest

from tests import meta_helpers as MH


def _digest(sc, nq, qseed):
    h = hashlib.sha256()
    Q, off, rows, desc = sc.queries(nq=nq, seed=qseed)
    for a in (sc.X, sc.node_ids, sc.mbits, sc.max_levels, Q, off, rows):
        h.update(str(a.dtype).encode() + str(a.shape).encode() + np.ascontiguousarray(a).tobytes())
    h.update(repr([tuple(None if v is None else (v if isinstance(v, str) else int(v)) for v in d) for d in desc]).encode())
    return h.hexdigest()


@pytest.mark.parametrize("seed,n,dim,nq,qseed,want", [
    (0, 400, 32, 24, 3, "4c198c7fc57524fba7c74317444d2d02bb30c57c8ab615804a8e31667629922b"),
    (11, 700, 48, 30, 5, "64cdd88e90e317c99711a5b152b2669d141a23513827eb815e6e1d9254c35b53"),
])
def test_default_scenario_is_bit_identical_to_the_two_field_original(seed, n, dim, nq, qseed, want):
    sc = MH.Scenario(n=n, dim=dim, seed=seed)
    assert (sc.mdim, sc.replicas) == (MH.MDIM, MH.REPLICAS) == (5, 4)
    assert _digest(sc, nq, qseed) == want
    assert [d[0] for d in sc.queries(nq=6)[3]] == ["is_color", "is_size", "and", "or", "neq_color", "mixed"]
    assert np.array_equal(sc.color, sc.values[0]) and np.array_equal(sc.size, sc.values[1])


@pytest.mark.parametrize("name,mdim,pseudo", [("A", 9, 73), ("B", 16, 60), ("C", 1, 2), ("D", 64, 22)])
def test_schema_shapes_and_query_kinds(name, mdim, pseudo):
    sc = MH.Scenario(n=50, dim=16, seed=1, **MH.SCHEMAS[name])
    nc = len(sc.conditions)
    assert sc.mdim == mdim and sc.mbits.shape == (50 * nc + pseudo, mdim)
    assert (sc.node_ids[:50 * nc] % sc.replicas >= 1).all() and (sc.node_ids[:50 * nc] % sc.replicas <= nc).all()
    assert (np.diff(sc.node_ids.astype(np.int64)) > 0).all() and sc.node_ids[50 * nc] == MH.PSEUDO_ROOT
    assert (sc.mbits[50 * nc] == 1).all()
    # every replica's dims are one pseudo node's dims (the node its condition and values select)
    pseudo_rows = {tuple(r) for r in sc.mbits[50 * nc + 1:].tolist()}
    assert len(pseudo_rows) == pseudo - 1 and all(tuple(r) in pseudo_rows for r in sc.mbits[:50 * nc].tolist())
    Q, off, rows, desc = sc.queries(nq=2 * (nc + 3), seed=2)
    assert rows.any(axis=1).all() and set(np.unique(rows)) <= {-1, 0, 1}        # never a Base-kind (all-zero) filter
    kinds = [d[0] for d in desc[:nc + 3]]
    assert kinds[nc:] == ["or", "neq_" + sc.names[sc.conditions[0][0]], "mixed"] and kinds[:nc] == list(sc.kind_cond)
    assert np.diff(off.astype(int)).tolist()[:nc + 3] == [1] * nc + [2, 1, 3]
    assert (rows[off[nc + 1]] != 0).sum() == sc.fields[sc.conditions[0][0]][1]      # NotEqual: every digit of the field is +-1
