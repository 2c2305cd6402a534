#!/usr/bin/env python3
"""cos_sparse_bruteforce_topk on the corpus and the 256 queries of scripts/bench_sparse.py (the handle keeps the raw rows here):
kernel time per batch next to cos_sparse_search_batch on the same handle, the scan's rate over the bytes of the raw CSR against the
streaming-read ceiling cos_hbm_probe reports, and recall@10 of the search against the exact answer at rerank factors 5 .. 100 (the
factors the wide pools admit at top_k 10).  Medians of RUNS runs of REPS calls with min - max.  One JSON line."""
import ctypes as C
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import cosdata_amd as ca
from cosdata_amd import _lib

n = int(os.environ.get("SPARSE_N", 400_000)); vocab = 30_000; nnz = 48; bits = 6; upper = 3.0; B = 256; k = 10
RUNS, REPS = 3, 5
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(3)
pz = 1.0 / torch.arange(1, vocab + 1, device=dev, dtype=torch.float64) ** 0.9
cdf = torch.cumsum(pz / pz.sum(), 0)
dim = torch.searchsorted(cdf, torch.rand(n * nnz, generator=g, device=dev, dtype=torch.float64)).clamp_(max=vocab - 1)
vid = torch.arange(n, device=dev).repeat_interleave(nnz)
key_pair = torch.unique(dim * n + vid)                                   # one posting per (dim, vector)
dim, vid = key_pair // n, key_pair % n
val = torch.exp(0.6 * torch.randn(dim.numel(), generator=g, device=dev)).clamp_(max=upper * 1.2).float()
order = torch.argsort(vid * vocab + dim)                                 # the raw rows: by vector, dimensions ascending
row_off = torch.zeros(n + 1, dtype=torch.int64, device=dev); row_off[1:] = torch.cumsum(torch.bincount(vid, minlength=n), 0)
ix = ca.InvertedIndex.from_vectors(bits, upper, row_off.cpu().numpy().astype(np.uint64), dim[order].cpu().numpy().astype(np.uint32),
                                   val[order].cpu().numpy())
ix.set_max_candidates(1024)
rng = np.random.default_rng(9)
pz_h = (pz / pz.sum()).cpu().numpy()
qd, qv, qo = [], [], [0]
for _ in range(B):
    m = int(rng.integers(16, 33))
    qd.append(np.sort(rng.choice(vocab, m, replace=False, p=pz_h)).astype(np.uint32))
    qv.append(np.exp(0.6 * rng.standard_normal(m)).astype(np.float32)); qo.append(qo[-1] + m)
qd, qv, qo = np.concatenate(qd), np.concatenate(qv), np.array(qo, np.uint32)


def med(calls):
    """median of RUNS medians of REPS calls, with the min and max of all calls"""
    runs = [[calls() for _ in range(REPS)] for _ in range(RUNS)]
    return {"median_ms": float(np.median([np.median(r) for r in runs])), "min_ms": float(np.min(runs)), "max_ms": float(np.max(runs))}


def brute_ms(kk):
    ix.bruteforce_topk(qd, qv, qo, kk)
    return ix.last_brute_stats()["kernel_ms"]


def search_ms(factor):
    ix.search_batch(qd, qv, qo, k, 0.0, factor)
    return ix.last_stats().kernel_ms


brute_ms(k); search_ms(5)  # warm both
out = {"config": {"workload": f"learned-sparse exact scan: {n} vectors, vocab {vocab}, {int(dim.numel())} raw pairs, batch {B} queries of 16-32 terms"}}
out["bruteforce_topk"] = {f"k{kk}": med(lambda: brute_ms(kk)) for kk in (10, 100, 1024)}
out["search_batch"] = {f"factor{f}": med(lambda: search_ms(f)) for f in (5, 100)}
st = ix.last_brute_stats()
gbps = C.c_double(0)
_lib.check(_lib.lib().cos_hbm_probe(0, 0, 1 << 30, 0, 10, C.byref(gbps)))
t = out["bruteforce_topk"]["k10"]["median_ms"] * 1e-3
passes = (B + 15) // 16  # every block of 16 queries streams the CSR once
out["roofline"] = {"raw_csr_bytes": int(st["raw_bytes"]), "hbm_read_ceiling_GBps": gbps.value, "one_pass_at_ceiling_ms": st["raw_bytes"] / gbps.value / 1e6,
                   "passes": passes, "achieved_GBps_one_pass": st["raw_bytes"] / t / 1e9, "achieved_GBps_all_passes": passes * st["raw_bytes"] / t / 1e9,
                   "slow_queries": int(st["slow_queries"]), "blocks": int(st["blocks"])}
truth, _, tc = ix.bruteforce_topk(qd, qv, qo, k)
out["recall_at_10"] = {}
for f in (5, 12, 25, 51, 100):  # 50 .. 1000 candidates: pools of 64, 128, 256, 512, 1024
    ids, _, cn = ix.search_batch(qd, qv, qo, k, 0.0, f)
    hit = sum(np.intersect1d(ids[b, :cn[b]], truth[b, :tc[b]]).size for b in range(B))
    out["recall_at_10"][f"factor{f}"] = hit / int(tc.sum())
print(json.dumps(out))
