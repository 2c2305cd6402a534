#!/usr/bin/env python3
"""cos_flat_search_f16_batch against the nearest path a HalfPrecisionFP index had before it, cos_bruteforce_topk with k = 50.

    timeout -k 10 600 python scripts/bench_flat_f16.py [--n 1000000] [--reps 10]

One process.  Per width (768, 1024): a Gaussian-mixture corpus of --n rows in an f16 index, 256 queries, top_k 10; a warm-up call, then
--reps timed calls of each path on the same handle, alternating; the median wall time of a call, the scan kernel's own time
(cos_flat_f16_stats::gemm_ms, HIP events), and that kernel's share of the f16 MFMA peak (2 B n dim flops) and of the HBM roof (the f16
rows, streamed once per 128 queries).  Then the masked call (cos_flat_search_f16_masked_batch) on the same handle: an all-ones mask beside
the unmasked call, 50 / 10 / 1 % live as random rows and as one contiguous id range (tiles_scanned / tiles_total, the scan kernel's
time), and exact_mode 2 at 1 % live against all live.  --masked 0 leaves that section out.  One JSON line."""
import argparse, json, os, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--masked", type=int, default=1)
ap.add_argument("--dims", type=int, nargs="+", default=[768, 1024])
ap.add_argument("--peak-tflops", type=float, default=2516.0, help="dense f16 MFMA peak of the device")
ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM roof of the device")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cosdata_amd as ca
from cosdata_amd.index import pack_row_masks

B, TOP_K = 256, 10


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


def masked_cases(ix, Q, n):
    """median wall / scan-kernel ms of the masked call per mask; the unmasked call is timed between the cases, as everywhere here"""
    rng, out = np.random.default_rng(4), {}
    def timed(mask, mode=1, Q=Q):
        call = (lambda: ix.flat_search_f16(Q, TOP_K, exact_mode=mode, with_stats=True)) if mask is None else \
               (lambda: ix.flat_search_f16_masked(Q, TOP_K, mask, exact_mode=mode, with_stats=True))
        call()
        ms, gemm = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            st = call()[3]
            ms.append((time.perf_counter() - t) * 1e3)
            gemm.append(st.gemm_ms)
        return {"ms": float(np.median(ms)), "min_max_ms": [float(np.min(ms)), float(np.max(ms))], "scan_kernel_ms": float(np.median(gemm)),
                "tiles": [int(st.tiles_scanned), int(st.tiles_total)], "exact_queries": int(st.exact_queries)}
    out["unmasked"] = timed(None)
    out["all_live"] = timed(pack_row_masks(np.ones(n, bool)))
    for pct in (50, 10, 1):
        out[f"random_{pct}"] = timed(pack_row_masks(rng.random(n) < pct / 100.0))
        rows = np.zeros(n, bool)
        rows[n // 3: n // 3 + n * pct // 100] = True
        out[f"range_{pct}"] = timed(pack_row_masks(rows))
    out["unmasked_again"] = timed(None)
    # the exact path (n * dim dependent additions per query and live row): eight queries, every row live against the 1 % range
    out["exact_all_live"] = timed(pack_row_masks(np.ones(n, bool)), 2, Q[:8])
    out["exact_range_1"] = timed(pack_row_masks(rows), 2, Q[:8])
    return out


cases = {}
for d in args.dims:
    X = clustered(args.n, d)
    rng = np.random.default_rng(8)
    Q = (X[rng.integers(0, args.n, B)] + np.float32(0.05) * rng.standard_normal((B, d), dtype=np.float32)).astype(np.float32)
    ix = ca.HNSWIndex(d, ca.HNSWHyperParams(num_layers=3), storage_type=ca.StorageType(ca.StorageKind(2), 0))
    ix.upload_vectors(X)
    ix.flat_search_f16(Q, TOP_K)
    ix.bruteforce_topk(Q, 5 * TOP_K)
    f16_ms, brute_ms, gemm_ms, exact = [], [], [], 0
    for _ in range(args.reps):
        t = time.perf_counter()
        st = ix.flat_search_f16(Q, TOP_K, with_stats=True)[3]
        f16_ms.append((time.perf_counter() - t) * 1e3)
        gemm_ms.append(st.gemm_ms)
        exact = max(exact, st.exact_queries)
        t = time.perf_counter()
        ix.bruteforce_topk(Q, 5 * TOP_K)
        brute_ms.append((time.perf_counter() - t) * 1e3)
    g = float(np.median(gemm_ms))
    row_bytes = (2 * d + 15) & ~15
    cases[f"{args.n}x{d} B{B} top_k{TOP_K}"] = {
        "flat_f16_ms": float(np.median(f16_ms)), "flat_f16_min_max_ms": [float(np.min(f16_ms)), float(np.max(f16_ms))],
        "bruteforce_k50_ms": float(np.median(brute_ms)), "bruteforce_min_max_ms": [float(np.min(brute_ms)), float(np.max(brute_ms))],
        "scan_kernel_ms": g, "exact_queries": int(exact),
        "mfma_peak_share": 2.0 * B * args.n * d / (g * 1e-3) / (args.peak_tflops * 1e12),
        "hbm_roof_share": args.n * row_bytes * ((B + 127) // 128) / (g * 1e-3) / (args.hbm_gbs * 1e9),
    }
    if args.masked:
        cases[f"{args.n}x{d} B{B} top_k{TOP_K}"]["masked"] = masked_cases(ix, Q, args.n)
    del ix, X
print(json.dumps({"reps": args.reps, "cases": cases}))
