#!/usr/bin/env python3
"""The learned-sparse half of a shard set on the index of scripts/bench_sparse.py — 360 000 SPLADE-shaped vectors,
~48 non-zero dimensions each over a Zipf vocabulary of 30 000, 6-bit keys, raw vectors resident — once as ONE handle and once as
8 id-range shards behind cos_shardset_sparse_search_batch, everything on ONE device.  256-query batches of 16-32 terms, top_k 10,
without a rerank (factor 0) and with one (factor 5, C = 50 candidates per query); wall clock of the host call (host arrays in, host
arrays out), the same bits asserted.  One JSON line.

    timeout -k 10 600 python scripts/bench_shardset_sparse.py

One device runs its shards' scans one after the other, so nothing here shows what S GPUs gain by scanning at once."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--vectors", type=int, default=360_000)
ap.add_argument("--shards", type=int, default=8)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--top-k", type=int, default=10)
ap.add_argument("--reps", type=int, default=10)
a = ap.parse_args()

import torch
import cosdata_amd as ca
from cosdata_amd import _lib
from cosdata_amd.shardset import ShardSet

n, S, B, k = a.vectors, a.shards, a.batch, a.top_k
vocab, nnz, bits, upper = 30_000, 48, 6, 3.0
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(3)
pz = 1.0 / torch.arange(1, vocab + 1, device=dev, dtype=torch.float64) ** 0.9
cdf = torch.cumsum(pz / pz.sum(), 0)
dim = torch.searchsorted(cdf, torch.rand(n * nnz, generator=g, device=dev, dtype=torch.float64)).clamp_(max=vocab - 1)
vid = torch.arange(n, device=dev).repeat_interleave(nnz)
pair = torch.unique(vid * vocab + dim)                                    # one pair per (vector, dim), vector-major, dims ascending in a row
vid, dim = pair // vocab, pair % vocab
val = torch.exp(0.6 * torch.randn(dim.numel(), generator=g, device=dev)).clamp_(max=upper * 1.2).float()
row_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
row_off[1:] = torch.cumsum(torch.bincount(vid, minlength=n), 0)
ro, rd, rv = row_off.cpu().numpy().astype(np.uint64), dim.cpu().numpy().astype(np.uint32), val.cpu().numpy()

rng = np.random.default_rng(9)
pz_h = (pz / pz.sum()).cpu().numpy()
qd, qv, qo = [], [], [0]
for _ in range(B):
    m = int(rng.integers(16, 33))
    qd.append(np.sort(rng.choice(vocab, m, replace=False, p=pz_h)).astype(np.uint32))
    qv.append(np.exp(0.6 * rng.standard_normal(m)).astype(np.float32)); qo.append(qo[-1] + m)
qd, qv, qo = np.concatenate(qd), np.concatenate(qv), np.array(qo, np.uint32)

t0 = time.perf_counter()
whole = ca.InvertedIndex.from_vectors(bits, upper, ro, rd, rv, keep_raw=True)
bounds = [n * s // S for s in range(S + 1)]
shards = []
for s in range(S):
    lo, hi = int(ro[bounds[s]]), int(ro[bounds[s + 1]])
    shards.append(ca.InvertedIndex.from_vectors(bits, upper, ro[bounds[s]:bounds[s + 1] + 1] - ro[bounds[s]], rd[lo:hi], rv[lo:hi], keep_raw=True))
X = np.random.default_rng(1).standard_normal((4, 8)).astype(np.float32)
stubs = [ca.HNSWIndex(8, ca.HNSWHyperParams(num_layers=3), id_base=int(b)).upload_vectors(X) for b in bounds[:-1]]
ss = ShardSet(stubs).attach_sparse(shards)
build_s = time.perf_counter() - t0


def wall(call):
    call(); call()
    ts = []
    for _ in range(a.reps):
        t = time.perf_counter(); out = call(); ts.append((time.perf_counter() - t) * 1e3)
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}, out


def same(x, y):
    return bool(np.array_equal(x[2], y[2]) and all(np.array_equal(x[0][q, :x[2][q]], y[0][q, :y[2][q]]) and
                                                    np.array_equal(x[1][q, :x[2][q]].view(np.uint32), y[1][q, :y[2][q]].view(np.uint32)) for q in range(B)))


out = {"bench": "shardset_sparse", "vectors": n, "pairs": int(rd.size), "shards": S, "batch": B, "top_k": k, "library": _lib.SO_PATH,
       "build_s": build_s, "ms_per_batch": {}}
for factor in (0, 5):
    one_ms, one = wall(lambda: whole.search_batch(qd, qv, qo, k, 0.0, factor))
    set_ms, got = wall(lambda: ss.sparse_search(qd, qv, qo, k, 0.0, factor))
    out["ms_per_batch"][f"factor_{factor}"] = {"one_handle": one_ms, f"set_of_{S}": set_ms, "same_bits": same(got, one)}
    assert same(got, one), f"factor {factor}: the set's answer is not the single handle's"
print(json.dumps(out))
