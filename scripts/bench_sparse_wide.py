#!/usr/bin/env python3
"""Learned-sparse search at 10 .. 1024 candidates per query (cos_sparse_set_max_candidates) on the corpus and the 256 queries of
scripts/bench_sparse.py, the raw vectors kept for the rerank legs.  One handle at 1024; per (top_k, reranking_factor) one warm-up
call and five timed ones: the median HIP-event time of the call's kernels, its ratio to the (64, 0) case, and the queries whose
ids, score bits or counts differ from the oracle (sequential_search cut to top_k x factor, raw-value rerank) over all 256 queries
of every case.  One JSON line; exit status 1 when any query mismatches.

    timeout -k 10 900 python scripts/bench_sparse_wide.py
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_sparse_wide.py --cases 1024,0 200,5 --no-parity
    timeout -k 10 300 python scripts/bench_sparse_wide.py --no-parity --lib /path/to/another/libcosdata_hip.so

The last form times another build of the library (the parent commit's, say) on the same corpus: run the two alternately."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import cosdata_amd as ca
from cosdata_amd import _lib
from oracle import oracle as O

CASES = [(10, 0), (64, 0), (65, 0), (128, 0), (256, 0), (512, 0), (1024, 0), (20, 5), (200, 5)]
ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="*", default=None, help="top_k,factor pairs (default: all nine)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-parity", action="store_true", help="skip the oracle (profiler runs)")
ap.add_argument("--lib", default=None, help="load this libcosdata_hip.so instead of the tree's")
args = ap.parse_args()
if args.lib:
    _lib.SO_PATH = os.path.abspath(args.lib)
cases = [tuple(int(x) for x in c.split(",")) for c in args.cases] if args.cases else CASES

n = int(os.environ.get("SPARSE_N", 400_000)); vocab = 30_000; nnz = 48; bits = 6; upper = 3.0; B = 256
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(3)
pz = 1.0 / torch.arange(1, vocab + 1, device=dev, dtype=torch.float64) ** 0.9
cdf = torch.cumsum(pz / pz.sum(), 0)
dim = torch.searchsorted(cdf, torch.rand(n * nnz, generator=g, device=dev, dtype=torch.float64)).clamp_(max=vocab - 1)
vid = torch.arange(n, device=dev).repeat_interleave(nnz)
key_pair = torch.unique(dim * n + vid)                                   # one posting per (dim, vector)
dim, vid = key_pair // n, key_pair % n
val = torch.exp(0.6 * torch.randn(dim.numel(), generator=g, device=dev)).clamp_(max=upper * 1.2).float()
Q = 1 << bits
qk = torch.clamp((val / upper * (Q - 1)).clamp(0, Q - 1).to(torch.int64), max=Q - 1)   # InvertedIndexNode::quantize (values >= 0)
order = torch.argsort((dim * Q + qk) * n + vid)
dim_s, qk_s, vid_s = dim[order], qk[order], vid[order]
dims_present = torch.unique(dim_s)
T = dims_present.numel()
cnt = torch.bincount(torch.searchsorted(dims_present, dim_s) * Q + qk_s, minlength=T * Q).view(T, Q)
key_off = torch.zeros(T, Q + 1, dtype=torch.int64, device=dev)
key_off[:, 1:] = torch.cumsum(cnt, 1)
base = torch.zeros(T, dtype=torch.int64, device=dev); base[1:] = torch.cumsum(cnt.sum(1), 0)[:-1]
key_off += base[:, None]
dims_h = dims_present.cpu().numpy().astype(np.uint32); ko_h = key_off.cpu().numpy().astype(np.uint64).ravel(); vid_h = vid_s.cpu().numpy().astype(np.uint32)
# the raw vectors, dimensions ascending inside a row
by_row = torch.argsort(vid * vocab + dim)
row_off = np.concatenate([[0], np.cumsum(torch.bincount(vid, minlength=n).cpu().numpy())]).astype(np.uint64)
raw_dims = dim[by_row].cpu().numpy().astype(np.uint32); raw_vals = val[by_row].cpu().numpy().astype(np.float32)
ix = ca.InvertedIndex(bits, upper, dims_h, ko_h, vid_h, n, row_off, raw_dims, raw_vals)
ix.set_max_candidates(1024)
rng = np.random.default_rng(9)
pz_h = (pz / pz.sum()).cpu().numpy()
qd, qv, qo = [], [], [0]
for _ in range(B):
    m = int(rng.integers(16, 33))
    d = np.sort(rng.choice(vocab, m, replace=False, p=pz_h)).astype(np.uint32)
    qd.append(d); qv.append(np.exp(0.6 * rng.standard_normal(m)).astype(np.float32)); qo.append(qo[-1] + m)
qd, qv, qo = np.concatenate(qd), np.concatenate(qv), np.array(qo, np.uint32)
thr = 0.0

results, got = {}, {}
for k, rf in cases:
    ix.search_batch(qd, qv, qo, k, thr, rf)
    kms = []
    for _ in range(args.reps):
        got[(k, rf)] = ix.search_batch(qd, qv, qo, k, thr, rf)
        kms.append(ix.last_stats().kernel_ms)
    st = ix.last_stats()
    results[f"{k},{rf}"] = {"kernel_ms": float(np.median(kms)), "kernel_ms_all": [round(float(x), 4) for x in kms], "blocks": int(st.blocks),
                            "postings_visited": int(st.postings_visited)}
if "64,0" in results:
    for r in results.values():
        r["ratio_to_64_0"] = r["kernel_ms"] / results["64,0"]["kernel_ms"]

total_bad = None
if not args.no_parity:
    from concurrent.futures import ThreadPoolExecutor
    import bench
    widest = max(k * max(rf, 1) for k, rf in cases)
    def one(b):   # the oracle's order is total (similarity, then id): the first m entries are its answer for k_with_reranking = m
        return O.sparse_search(dims_h, ko_h, vid_h, n, bits, upper, thr, qd[qo[b]:qo[b + 1]], qv[qo[b]:qo[b + 1]], k_with_reranking=widest)
    with ThreadPoolExecutor(min(bench.effective_cores(), 16)) as ex:
        ref = list(ex.map(one, range(B)))
    total_bad = 0
    for k, rf in cases:
        ids, sc, cnt_o = got[(k, rf)]
        bad = 0
        for b in range(B):
            cand, sims = ref[b][0][:k * max(rf, 1)], ref[b][1][:k * max(rf, 1)]
            if rf:
                eid, esc = O.sparse_rerank(row_off, raw_dims, raw_vals, cand, qd[qo[b]:qo[b + 1]], qv[qo[b]:qo[b + 1]], top_k=k)
            else:
                eid, esc = cand[:k], sims[:k].astype(np.float32)
            c = int(cnt_o[b])
            bad += not (c == len(eid) and np.array_equal(ids[b, :c], eid)
                        and np.array_equal(sc[b, :c].view(np.uint32), np.asarray(esc, np.float32).view(np.uint32)))
        results[f"{k},{rf}"]["mismatching_queries"] = int(bad)
        total_bad += bad
print(json.dumps({"config": {"workload": f"learned-sparse inverted index, {n} vectors, vocab {vocab}, {int(dim.numel())} postings, {bits}-bit keys, "
                                         f"batch {B} queries of 16-32 terms, handle at max_candidates {ix.max_candidates}",
                             "layout": "packed u32" if ix.packed else "u32 id + u8 key", "timed_calls": args.reps,
                             "library": _lib.SO_PATH},
                  "cases": results, "parity_vs_oracle": {"queries_per_case": B, "mismatching_queries": total_bad}}))
sys.exit(1 if total_bad else 0)
