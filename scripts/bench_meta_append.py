#!/usr/bin/env python3
"""Appending to a collection with a metadata schema at the size DESIGN.md quotes for the component (600 k nodes): a collection of N0
embeddings with the two-field schema of tests/meta_helpers.py (3 replicas + 24 pseudo nodes) takes 10 % more embeddings with their
replicas.  Times cos_index_append + cos_index_append_meta against what the same library's cos_index_build + cos_index_build_meta take
for the grown collection (the only path before cos_index_append accepted such a collection), and cos_search_filtered_batch before the
append, after it, and on the rebuilt collection that no append touched.  One JSON line."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cosdata_amd as ca
from tests import meta_helpers as MH

N0 = int(os.environ.get("META_N", 200_000)); N1 = N0 + N0 // 10; DIM = int(os.environ.get("META_DIM", 768)); B = 256; REPS = 10
# Layers: with the 6 of the small test scenarios the top mixed level of 600 k nodes holds thousands of replicas, the pseudo nodes' slots
# fill up with them and evict their edges to the pseudo root (prob_node.rs:271-279) — most walks from the root then find nothing, and an
# append that links nothing measures nothing.  10 layers leave a handful of replicas on the top mixed level, as at test size.
LAYERS = int(os.environ.get("META_LAYERS", 10))
out = {"config": {"workload": f"metadata collection {N0} -> {N1} x {DIM} u8, 3 Metadata replicas per embedding, 5 metadata dimensions, {LAYERS} layers, batch {B}"}}

sc = MH.Scenario(n=N1, dim=DIM, seed=5, ef_search=64, num_layers=LAYERS)
p = sc.params
pseudo = sc.node_ids >= MH.PSEUDO_ROOT
old = pseudo | (sc.node_ids // sc.replicas < N0)
table = lambda m: (sc.node_ids[m], sc.mbits[m], sc.max_levels[m])
Q, off, rows, _ = sc.queries(nq=B, seed=3)
fd = rows.astype(np.int8)


def handle(X):
    h = ca.HNSWHyperParams(num_layers=p.num_layers, ef_construction=p.ef_construction, ef_search=p.ef_search,
                           level_0_neighbors_count=p.level0_neighbors_count, neighbors_count=p.neighbors_count)
    dix = ca.HNSWIndex(DIM, h, ca.DistanceMetric(p.metric), ca.StorageType(ca.StorageKind(p.storage), p.resolution), (p.range_lo, p.range_hi), p.shortlist_size,
                       seed=p.seed)
    dix.upload_vectors(X).enable_metadata(sc.mdim, sc.replicas)
    return dix


def timed(f):
    t = time.perf_counter()
    f()                                                        # (every call waits for the device before it returns)
    return time.perf_counter() - t


def search_ms(dix):
    dix.search_filtered(Q, off, fd, 10)
    runs = []
    for _ in range(REPS):
        t = time.perf_counter()
        res = dix.search_filtered(Q, off, fd, 10)
        runs.append((time.perf_counter() - t) * 1e3)
    return {"ms_per_batch_host_api_median": float(np.median(runs)), "min": float(min(runs)), "max": float(max(runs)),
            "queries_with_results": int((res[2] > 0).sum())}, res


# ---- the collection before the commit of new documents -----------------------------------------------------------------------------
a = handle(sc.X[:N0])
out["old_collection"] = {"build_s": timed(lambda: a.build(4096)), "build_meta_s": timed(lambda: a.build_meta(*table(old), 0)),
                         "component_nodes": int(old.sum())}
out["filtered_search_before_append"], _ = search_ms(a)

# ---- append: the embeddings, then their replica nodes --------------------------------------------------------------------------------
t_append = timed(lambda: a.append(sc.X[N0:], 4096))
t_append_meta = timed(lambda: a.append_meta(*table(~old), 0))
out["append"] = {"embeddings": N1 - N0, "replica_nodes": int((~old).sum()), "append_s": t_append, "append_meta_s": t_append_meta,
                 "total_s": t_append + t_append_meta}
out["filtered_search_after_append"], res_a = search_ms(a)
def connectivity(dix):
    """level 0 of the component: nodes, nodes without any neighbour among the old and among the appended replicas, the pseudo root's degree"""
    ids, nbr = dix.download_meta_graph()[0]
    lone = ~(nbr != ca.SLOT_EMPTY).any(axis=1)
    new = np.isin(ids, sc.node_ids[~old])
    return {"nodes": int(ids.size), "old_without_neighbour": int((lone & ~new).sum()), "appended_without_neighbour": int((lone & new).sum()),
            "pseudo_root_degree": int((nbr[np.searchsorted(ids, MH.PSEUDO_ROOT)] != ca.SLOT_EMPTY).sum())}


out["append"]["level0_after"] = connectivity(a)
del a

# ---- the path there was before: build the grown collection from scratch ---------------------------------------------------------------
b = handle(sc.X)
t_build = timed(lambda: b.build(4096))
t_build_meta = timed(lambda: b.build_meta(sc.node_ids, sc.mbits, sc.max_levels, 0))
out["rebuild"] = {"build_s": t_build, "build_meta_s": t_build_meta, "total_s": t_build + t_build_meta, "component_nodes": int(sc.node_ids.size)}
out["filtered_search_rebuilt_untouched"], res_b = search_ms(b)
out["rebuild"]["level0"] = connectivity(b)
out["append_vs_rebuild_speedup"] = out["rebuild"]["total_s"] / out["append"]["total_s"]
# the two collections hold the same nodes linked in different batch orders: how far their answers agree (not an equality claim)
same = [len(set(res_a[0][q, :res_a[2][q]]) & set(res_b[0][q, :res_b[2][q]])) / max(1, int(res_b[2][q])) for q in range(B)]
out["top10_overlap_appended_vs_rebuilt"] = float(np.mean(same))
print(json.dumps(out))
