#!/usr/bin/env python3
"""cos_flat_search_f32_batch against the two exhaustive answers that were there before it, in one process.

    timeout -k 10 1100 python scripts/bench_flat_f32.py [--n 1000000] [--reps 3]

Per width (768, 1024): a Gaussian-mixture corpus of --n rows uploaded into a FullPrecisionFP handle and a HalfPrecisionFP handle (half
the bytes); 256 queries.  Per top_k (10, 100): a warm-up call of every case, then --reps rounds that alternate the cases — the f32
call unmasked, with an all-ones mask and with a 1 % random mask, cos_bruteforce_topk on the f32 handle (the only exhaustive f32 answer
before this call; it keeps no event times, so only its host time is reported) and cos_flat_search_f16_batch on the f16 handle.  Per case
the median host time around the call (it ends in a synchronise), the median of the scan kernels' own time
(cos_flat_f16_stats::gemm_ms, HIP events), min and max of both, and the queries that took the exact pass.  `f32_spread_ms` is max - min
of the unmasked f32 call's kernel time over the rounds: what a difference has to exceed to mean anything.  One JSON line."""
import argparse, json, os, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
ap.add_argument("--top-k", type=int, nargs="+", default=[10, 100])
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cosdata_amd as ca
from cosdata_amd.index import pack_row_masks

B = 256


def clustered(n, d, n_centers=64, sigma=0.15, seed=3):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((n_centers, d), dtype=np.float32)
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    x = centers[rng.integers(0, n_centers, n)]
    for r0 in range(0, n, 65536):  # in place, block by block: the corpus is 4 GB at 1M x 1024
        blk = x[r0:r0 + 65536]
        blk += np.float32(sigma) * rng.standard_normal(blk.shape, dtype=np.float32)
        blk /= np.linalg.norm(blk, axis=1, keepdims=True)
    return x


def index(X, kind):
    return ca.HNSWIndex(X.shape[1], ca.HNSWHyperParams(num_layers=3), ca.DistanceMetric.Cosine, ca.StorageType(ca.StorageKind(kind), 0)).upload_vectors(X)


cases = {}
for d in args.dims:
    X = clustered(args.n, d)
    rng = np.random.default_rng(8)
    Q = (X[rng.integers(0, args.n, B)] + np.float32(0.05) * rng.standard_normal((B, d), dtype=np.float32)).astype(np.float32)
    f32_ix, f16_ix = index(X, 3), index(X, 2)
    ones, one_pct = pack_row_masks(np.ones(args.n, bool)), pack_row_masks(np.random.default_rng(4).random(args.n) < 0.01)
    for top_k in args.top_k:
        calls = {"f32": lambda: f32_ix.flat_search_f32(Q, top_k, with_stats=True)[3],
                 "f32_all_ones_mask": lambda: f32_ix.flat_search_f32(Q, top_k, ones, with_stats=True)[3],
                 "f32_1pct_mask": lambda: f32_ix.flat_search_f32(Q, top_k, one_pct, with_stats=True)[3],
                 "bruteforce_topk": lambda: f32_ix.bruteforce_topk(Q, top_k) and None,
                 "f16": lambda: f16_ix.flat_search_f16(Q, top_k, with_stats=True)[3]}
        host, kern, stats = {k: [] for k in calls}, {k: [] for k in calls}, {}
        for call in calls.values():
            call()
        for _ in range(args.reps):
            for name, call in calls.items():
                t = time.perf_counter()
                st = call()
                host[name].append((time.perf_counter() - t) * 1e3)
                if st is not None:
                    kern[name].append(st.gemm_ms)
                    stats[name] = st
        out = {}
        for name in calls:
            out[name] = {"host_ms": float(np.median(host[name])), "host_min_max_ms": [float(np.min(host[name])), float(np.max(host[name]))]}
            if name in stats:
                st = stats[name]
                out[name].update({"scan_kernel_ms": float(np.median(kern[name])), "scan_kernel_min_max_ms": [float(np.min(kern[name])), float(np.max(kern[name]))],
                                  "exact_queries": int(st.exact_queries), "pool": int(st.pool), "launches": int(st.gemm_launches),
                                  "tiles": [int(st.tiles_scanned), int(st.tiles_total)]})
        out["f32_spread_ms"] = float(np.max(kern["f32"]) - np.min(kern["f32"]))
        cases[f"{args.n}x{d} B{B} top_k{top_k}"] = out
    del f32_ix, f16_ix, X
print(json.dumps({"reps": args.reps, "cases": cases}))
