#!/usr/bin/env python3
"""cos_bruteforce_topk_dot beside cos_bruteforce_topk — the yardstick: both stream the same rows and issue the same MFMAs — on one
clustered corpus whose row norms vary by 4x.  Per shape (rows x dim) and k: two warm-up calls each, then `--reps` rounds of one cosine
call and one inner-product call, alternating; the median, the fastest and the slowest HOST-CLOCK time of a call (upload of the
queries, scan, selection, re-score, copies back), and the share of queries the inner product's margin rule sent down the exact pass.
The inner-product answer of a sample of the queries is compared with float64 scores (rank by rank, within the bound of
flat_plan.h).  One JSON line; exit status 1 on any mismatch.

    timeout -k 10 600 python scripts/bench_brute_dot.py
    timeout -k 10 300 python scripts/bench_brute_dot.py --n 1000000 --dims 768 --k 10"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--dims", type=int, nargs="*", default=[768, 1024])
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--k", type=int, nargs="*", default=[10, 100])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sample", type=int, default=4, help="queries checked against float64")
args = ap.parse_args()

import torch
import cosdata_amd as ca

n, B = args.n, args.batch
dev = torch.device("cuda:0")


def draw(m, d, centers, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    out = torch.empty(m, d, device=dev)
    for s in range(0, m, 1 << 18):
        c = min(1 << 18, m - s)
        idx = torch.randint(0, centers.shape[0], (c,), generator=g, device=dev)
        rows = (centers[idx] + 0.2 * torch.randn(c, d, generator=g, device=dev)).clamp_(-0.999, 0.999)
        out[s:s + c] = rows * (0.5 + 1.5 * torch.rand(c, 1, generator=g, device=dev))  # norms vary: the two rankings differ
    return out


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "ms_all": [round(x, 3) for x in ms]}


results, bad_total = {}, 0
for d in args.dims:
    g = torch.Generator(device=dev); g.manual_seed(7)
    centers = torch.rand(max(64, n // 1000), d, generator=g, device=dev) * 1.6 - 0.8
    X = draw(n, d, centers, 42)
    Qh = draw(B, d, centers, 43).cpu().numpy()
    torch.cuda.synchronize()
    ix = ca.HNSWIndex(d, ca.HNSWHyperParams(), ca.DistanceMetric.DotProduct, ca.StorageType.UnsignedByte(), (-2.0, 2.0))
    ix.upload_vectors_device(X.data_ptr(), n, keepalive=X)
    sample = np.linspace(0, B - 1, min(args.sample, B)).astype(int)
    S = (X.double() @ torch.from_numpy(Qh[sample]).to(dev).double().T).T.cpu().numpy()  # float64 scores of the sampled queries
    xn = float(X.double().norm(dim=1).max())
    c = 2.0 * ((d + d // 8 + 32) + 8) * 2.0 ** -24
    for k in args.k:
        for _ in range(2):
            ix.bruteforce_topk(Qh, k); ix.bruteforce_topk_dot(Qh, k)
        cos_ms, dot_ms, out = [], [], None
        for _ in range(args.reps):
            t = time.perf_counter(); ix.bruteforce_topk(Qh, k); cos_ms.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter(); out = ix.bruteforce_topk_dot(Qh, k); dot_ms.append((time.perf_counter() - t) * 1e3)
        st = ix.last_brute_stats()
        bad = 0
        for j, b in enumerate(sample):
            order = np.lexsort((-np.arange(n), -S[j]))[:k]
            tol = c * float(np.linalg.norm(Qh[b].astype(np.float64))) * xn
            got = out[0][b].astype(np.int64)  # (two float64 neighbours closer than the f32 error may come back swapped: scores are compared)
            bad += not (np.unique(got).size == k and np.all(np.abs(out[1][b].astype(np.float64) - S[j, got]) <= tol)
                        and np.all(np.abs(S[j, got] - S[j, order]) <= tol))
        bad_total += bad
        results[f"{n} x {d} k {k}"] = {"pool": int(st.pool), "cosine": stats(cos_ms), "dot": stats(dot_ms),
                                       "dot_exact_query_share": st.exact_queries / st.queries, "mismatching_sampled_queries": int(bad)}
    del ix, X

print(json.dumps({"config": {"workload": f"{n} clustered rows, norms 0.5x .. 2x, {B}-query calls, 2 warm-up + {args.reps} alternating timed calls per case",
                             "clock": "host clock around the call"}, "cases": results, "mismatching_sampled_queries": int(bad_total)}))
sys.exit(1 if bad_total else 0)
