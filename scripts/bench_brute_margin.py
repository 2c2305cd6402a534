#!/usr/bin/env python3
"""What the brute force's margin rule costs on ordinary data, and what its exact path costs where everything is flagged.

    timeout -k 10 300 python scripts/bench_brute_margin.py                       # this tree
    timeout -k 10 300 python scripts/bench_brute_margin.py --tree /path/to/parent  # another checkout (built), same corpora

One run = one process: per shape a warm-up call, then `--reps` timed cos_bruteforce_topk calls with default knobs, the median wall
time of a call.  Shapes: (70000, 96, B 37) and (20000, 768, B 130) Gaussian mixtures at k 10 — the rule flags nothing there, so the
tree differs from its parent by one launch of one thread per query and four more bytes in a copy it already made.  With --exact also
5000 x 64 where every row is a scaled copy of one vector (12 queries, k 10): every query takes the exact path (a tree without the
rule returns a wrong list there, in less time).  Alternate the two trees, three runs each, and compare the tree's median run with
the parent's slowest.  One JSON line per run."""
import argparse, json, os, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--exact", action="store_true")
ap.add_argument("--label", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import numpy as np
import cosdata_amd as ca
from cosdata_amd import _lib


def clustered(n, d, n_centers=20, sigma=0.15, seed=3):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((n_centers, d)).astype(np.float32)
    centers /= np.linalg.norm(centers, axis=1, keepdims=True)
    x = centers[rng.integers(0, n_centers, n)] + sigma * rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def queries(X, B, seed=8):
    rng = np.random.default_rng(seed)
    return (X[rng.integers(0, X.shape[0], B)] + 0.05 * rng.standard_normal((B, X.shape[1])).astype(np.float32)).astype(np.float32)


def timed(ix, Q, k):
    ix.bruteforce_topk(Q, k)
    ms = []
    for _ in range(args.reps):
        t = time.perf_counter()
        ix.bruteforce_topk(Q, k)
        ms.append((time.perf_counter() - t) * 1e3)
    out = {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}
    if hasattr(ix, "last_brute_stats"):
        out["exact_queries"] = int(ix.last_brute_stats().exact_queries)
    return out


cases = {}
for n, d, B in ((70000, 96, 37), (20000, 768, 130)):
    X = clustered(n, d)
    ix = ca.HNSWIndex(d, ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType.UnsignedByte())
    ix.upload_vectors(X)
    cases[f"{n}x{d} B{B} k10"] = timed(ix, queries(X, B), 10)
    del ix
if args.exact:
    base = clustered(5000, 64)[17]
    X = (base[None, :] * np.random.default_rng(6).uniform(0.5, 2.0, 5000).astype(np.float32)[:, None]).astype(np.float32)
    Q = np.concatenate([base[None, :] + np.float32(0.02) * np.random.default_rng(7).standard_normal((11, 64)).astype(np.float32), base[None, :]]).astype(np.float32)
    ix = ca.HNSWIndex(64, ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType.UnsignedByte())
    ix.upload_vectors(X)
    cases["5000x64 all scaled copies B12 k10"] = timed(ix, Q, 10)
print(json.dumps({"label": args.label or os.path.abspath(args.tree), "library": _lib.SO_PATH, "reps": args.reps, "cases": cases}))
