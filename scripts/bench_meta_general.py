#!/usr/bin/env python3
"""walk_meta_general_kernel (kernels_meta_general.hip) against walk_meta_kernel on the same work, and on the rows only it serves: a
256-query filtered batch on a metadata collection of META_N embeddings (two-field schema of tests/meta_helpers.py, 3 Metadata replicas
per embedding), u8 codes, built on the device:
    3072 dims                     only the general kernel runs
    2048 dims                     the fast kernel (default dispatch) and the general one (tuning knob meta_walk_general = 1)
The 2048-dim pair is the comparison: the two variants alternate call by call on ONE handle, after a warm-up of both; a time is the
host clock around cos_search_filtered_batch, which ends in a device synchronise (upload of the queries, quantisation, walk, finalize,
download: the same for both variants but for the walk).  Prints one JSON line per collection."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cosdata_amd as ca
from cosdata_amd import _lib
from tests import meta_helpers as MH

N = int(os.environ.get("META_N", 100_000)); B = 256; REPS = int(os.environ.get("META_REPS", 20)); LAYERS = int(os.environ.get("META_LAYERS", 10))


def collection(dim):
    sc = MH.Scenario(n=N, dim=dim, seed=5, ef_search=64, num_layers=LAYERS)      # (10 layers: see scripts/bench_meta_append.py)
    p = sc.params
    h = ca.HNSWHyperParams(num_layers=p.num_layers, ef_construction=p.ef_construction, ef_search=p.ef_search,
                           level_0_neighbors_count=p.level0_neighbors_count, neighbors_count=p.neighbors_count)
    dix = ca.HNSWIndex(dim, h, ca.DistanceMetric(p.metric), ca.StorageType(ca.StorageKind(p.storage), p.resolution), (p.range_lo, p.range_hi),
                       p.shortlist_size, seed=p.seed)
    dix.upload_vectors(sc.X).enable_metadata(sc.mdim, sc.replicas)
    t = time.perf_counter()
    dix.build(4096)
    t_build = time.perf_counter() - t
    t = time.perf_counter()
    dix.build_meta(sc.node_ids, sc.mbits, sc.max_levels, 0)
    Q, off, rows, _ = sc.queries(nq=B, seed=3)
    return dix, (Q, off, rows.astype(np.int8)), {"build_s": t_build, "build_meta_s": time.perf_counter() - t, "component_nodes": int(sc.node_ids.size)}


def one(dix, q, general):
    with _lib.tuning(meta_walk_general=int(general)):
        t = time.perf_counter()
        res = dix.search_filtered(*q, 10)
        return (time.perf_counter() - t) * 1e3, res


def summary(ms, res):
    return {"ms_per_batch_host_api_median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "queries_with_results": int((res[2] > 0).sum())}


for dim, variants in ((3072, (True,)), (2048, (False, True))):
    dix, q, built = collection(dim)
    out = {"workload": f"metadata collection {N} x {dim} u8, {B}-query filtered batch, ef_search 64, median of {REPS}", **built}
    for g in variants * 3:
        one(dix, q, g)                                           # warm-up of every variant
    runs = {g: [] for g in variants}
    last = {}
    for _ in range(REPS):
        for g in variants:                                       # alternating
            ms, last[g] = one(dix, q, g)
            runs[g].append(ms)
    for g in variants:
        out["general_kernel" if g else "fast_kernel"] = summary(runs[g], last[g])
    if len(variants) == 2:
        (fi, fs, fc), (gi, gs, gc) = last[False][:3], last[True][:3]
        same = np.array_equal(fc, gc) and all(np.array_equal(fi[b, :fc[b]], gi[b, :fc[b]]) and np.array_equal(fs[b, :fc[b]], gs[b, :fc[b]]) for b in range(B))
        out["same_answers"] = bool(same)
        out["general_over_fast"] = out["general_kernel"]["ms_per_batch_host_api_median"] / out["fast_kernel"]["ms_per_batch_host_api_median"]
    print(json.dumps(out), flush=True)
    del dix
