"""Independent restatement of the FILTERED ann_search in pure Python (small cases only), run against the C oracle on the
metadata components it built: the (node kind, query kind) arms of CosineSimilarity::calculate (distance/cosine.rs:36-102,
243-262) and the control flow of ann_search with query_filter_dims (vector_store.rs:256-402) over traverse_find_nearest
(vector_store.rs:1112-1204), written straight from the reference — one PerformantFixedSet per level shared by the walks of
every filter of the query (query id pre-seeded, the entry node evaluated whatever the set says), one heap walk per filter,
-1.0 dropped under the cosine metric only, keep-100 per walk and again over the level, the entry node with its strongest match
when nothing is left, descent through the best hit's child.  Vector distances come from the oracle's operator (pinned in
test_oracle_kat.py); the metadata arithmetic is small-integer f32 and is done here in numpy.  Nothing else is shared with
cosdata_oracle_hnsw.c.  Search only: the graphs are the oracle builder's."""
import heapq

import numpy as np
import pytest

from oracle import oracle as O
from tests import meta_helpers as MH

PSEUDO_LO, PSEUDO_HI = 0xFFFFFFFF - 257, 0xFFFFFFFF - 2          # metadata/mod.rs:217-224
BASE, PSEUDO, METADATA = range(3)


def _mag(mb):
    return np.sqrt(np.float32(sum(int(x) * int(x) for x in mb)))   # types.rs:112-146 (entries are -1, 0, 1: the sum is exact)


def _kind(mag, nid):
    """VectorData::replica_node_kind (types.rs:219-241); nid None = a search query"""
    if mag == 0.0:
        return BASE
    return PSEUDO if nid is not None and PSEUDO_LO <= nid <= PSEUDO_HI else METADATA


def _mdims_cos(a, amag, b, bmag):
    den = np.float32(amag) * np.float32(bmag)
    assert den != 0.0
    return np.float32(sum(int(x) * int(y) for x, y in zip(a, b))) / den


def _py_ann_search_filtered(levels, node_ids, mbits, codes, mags, qcode, qmag, filters, p, stride, n_vec):
    """levels[l] = (node ids ascending, nbr ids [n][M_l]) of the pseudo-root component; codes row n_vec = the all-zero vector every
    pseudo node shares.  Returns (ids, sims, per-level counts), top level first."""
    table = {int(i): k for k, i in enumerate(node_ids.tolist())}
    node_mag = [_mag(r) for r in mbits.tolist()]
    row = lambda nid: n_vec if PSEUDO_LO <= nid <= PSEUDO_HI else nid // stride
    fl = [(list(map(int, f)), _mag(f)) for f in filters]

    def vec(nid, metric):
        rc, v = O.distance(metric, p.storage, p.resolution, p.dim, qcode, qmag, codes[row(nid)], mags[row(nid)])
        assert rc == O.OK
        return np.float32(v)

    def dist(nid, f):
        fb, fmag = fl[f]
        if p.metric != O.METRIC_COSINE:                            # only CosineSimilarity looks at the node kinds
            return vec(nid, p.metric)
        k = table[nid]
        yk, xk = _kind(node_mag[k], nid), _kind(fmag, None)
        if (yk, xk) == (PSEUDO, METADATA):
            return np.float32(1.0 if fb == mbits[k].tolist() else -1.0)
        if (yk, xk) == (METADATA, METADATA):
            return vec(nid, O.METRIC_COSINE) if _mdims_cos(fb, fmag, mbits[k], node_mag[k]) > np.float32(0.99) else np.float32(-1.0)
        if (yk, xk) == (BASE, METADATA):
            return np.float32(0.0)
        raise AssertionError(f"unreachable arm {(yk, xk)}")

    order = lambda t: (float(t[0]), t[1])                          # similarity, then the larger id (the oracle's documented tie-break)
    out_ids, out_sims, counts = [], [], []
    entry = PSEUDO_LO
    for level in range(p.num_layers, -1, -1):
        ids, nbr = levels[level]
        pos = {int(v): i for i, v in enumerate(ids.tolist())}
        M = p.level0_neighbors_count if level == 0 else p.neighbors_count
        key = lambda v: v & (64 * M - 1)                           # fixedset.rs: plain id bits
        visited = {key(O.QUERY_ID)}                                # vector_store.rs:266-271, ONE set for all the filters
        z = []
        for f in range(len(fl)):
            s0 = dist(entry, f)                                    # :1144 before any look at the set
            visited.add(key(entry))
            heap = [(-float(s0), -entry, entry, s0)]
            popped = []
            while heap:
                _, _, node, s = heapq.heappop(heap)
                if len(popped) >= p.ef_search:
                    break
                popped.append((s, node))
                for j in range(min(M, p.shortlist_size)):
                    nid = int(nbr[pos[node], j])
                    if nid == O.SLOT_EMPTY or key(nid) in visited:
                        continue
                    d = dist(nid, f)
                    visited.add(key(nid))
                    heapq.heappush(heap, (-float(d), -nid, nid, d))
            popped.sort(key=order, reverse=True)
            for s, node in popped[:100]:                           # :293-304
                if p.metric == O.METRIC_COSINE and s == np.float32(-1.0):
                    continue
                z.append((s, node))
        z.sort(key=order, reverse=True)
        z = z[:100]
        if not z:                                                  # :329-380
            z = [max(((dist(entry, f), entry) for f in range(len(fl))), key=order)]
        out_ids += [t[1] for t in z]
        out_sims += [t[0] for t in z]
        counts.append(len(z))
        entry = z[0][1]                                            # child = the same id one level down
    return np.array(out_ids, np.uint32), np.array(out_sims, np.float32), np.array(counts, np.uint32)


@pytest.fixture(scope="module", params=["A", "B", "D"])
def world(request):
    sc = MH.Scenario(n=300, dim=32, seed=6, **MH.SCHEMAS[request.param])
    oix = sc.oracle()
    codes, mags = O.quantize_batch(np.vstack([sc.X, np.zeros((1, sc.dim), np.float32)]), sc.params.storage, 0, -1.0, 1.0)
    return sc, oix, oix.meta_export_graph(), codes, mags


@pytest.mark.parametrize("ef", [3, 24, 120])
def test_python_filtered_walk_equals_c_oracle(world, ef):
    sc, oix, levels, codes, mags = world
    oix.set_ef_search(ef)
    p = sc.params
    assert p.ef_search == ef
    Q, off, rows, desc = sc.queries(nq=8, seed=ef)
    fallbacks = hits = 0
    for b in range(8):
        f = rows[off[b]:off[b + 1]]
        qcode, qmag = O.quantize(Q[b], p.storage, p.resolution, -1.0, 1.0)
        pi, ps, pc = _py_ann_search_filtered(levels, sc.node_ids, sc.mbits, codes, mags, qcode, qmag, f, p, sc.replicas, sc.n)
        ci, cs, cc = oix.ann_search_filtered(Q[b], f)
        assert np.array_equal(pc, cc), (desc[b], pc, cc)
        assert np.array_equal(pi, ci), desc[b]
        assert np.array_equal(ps.view(np.uint32), cs.view(np.uint32)), desc[b]
        fallbacks += int(((cc == 1) & (cs[np.cumsum(cc) - cc] == -1.0)).sum())
        hits += int((ci < PSEUDO_LO).any())
    assert hits >= 3                                               # walks do reach replicas, and (below) levels do fall back
    assert fallbacks >= 1
