#!/usr/bin/env python3
"""What one shard-set call saves a host that shards its collection: S = 8 id-range shards of one clustered corpus on ONE device, 256-query
calls.  Per operator the new call (cos_shardset_bruteforce_topk, cos_shardset_flat_search_batch, cos_shardset_search_filtered_batch:
per-shard records stay on the device, one exchange, one merge kernel, one copy back) against the only path before it: the S
single-index host calls in a row plus a merge in numpy.  Then the wide merge alone (cos_merge_lists_packed_device) at 2048, 4096 and
8192 keys per query, HIP-event time per launch.  Per case two warm-up calls and `--reps` timed ones: median and min-max wall time.  One
JSON line.

    timeout -k 10 900 python scripts/bench_shardset_modes.py

One device runs its shards in turn, so nothing here shows what S GPUs gain by scanning at once (one host thread per device): the
numbers are the saved copies and the host merge only."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=800_000)
ap.add_argument("--dim", type=int, default=256)
ap.add_argument("--shards", type=int, default=8)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--filtered-n", type=int, default=1500, help="embeddings per shard of the metadata collection (0 = skip the filtered case)")
args = ap.parse_args()

import torch
import cosdata_amd as ca
from cosdata_amd import _lib
from cosdata_amd.shardset import ShardSet
from cosdata_amd.sharding import merge_lists_packed_device, shard_range

n, d, S, B = args.n, args.dim, args.shards, args.batch
rng = np.random.default_rng(7)
centers = rng.uniform(-0.8, 0.8, (max(64, n // 1000), d)).astype(np.float32)


def draw(m, seed):
    r = np.random.default_rng(seed)
    return np.clip(centers[r.integers(0, len(centers), m)] + 0.2 * r.standard_normal((m, d)).astype(np.float32), -0.999, 0.999).astype(np.float32)


X, Q = draw(n, 42), draw(B, 43)


def host_merge(parts, k):
    """the host's own S-way merge, vectorised: total_cmp score descending, larger id first"""
    ids = np.concatenate([p[0] for p in parts], axis=1).astype(np.uint64)
    bits = np.concatenate([p[1] for p in parts], axis=1).view(np.uint32)
    key = np.where(bits >> 31, ~bits, bits | np.uint32(0x80000000)).astype(np.uint64)
    live = np.concatenate([np.arange(k)[None, :] < np.asarray(p[2])[:, None] for p in parts], axis=1)
    packed = np.where(live, (key << np.uint64(32)) | ids, np.uint64(0))
    top = np.sort(packed, axis=1)[:, ::-1][:, :k]
    kb = (top >> np.uint64(32)).astype(np.uint32)
    sc = np.where(kb >> 31, kb & np.uint32(0x7FFFFFFF), ~kb).view(np.float32)
    return (top & np.uint64(0xFFFFFFFF)).astype(np.uint32), sc, np.minimum(live.sum(axis=1), k).astype(np.uint32)


def timed(call):
    call(); call()
    wall = []
    for _ in range(args.reps):
        t = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t) * 1e3)
    return {"ms_per_call": float(np.median(wall)), "ms_min": float(min(wall)), "ms_max": float(max(wall))}, out


def pair(one_call, per_shard, k):
    new, a = timed(one_call)
    old, b = timed(lambda: host_merge(per_shard(), k))
    same = bool(np.array_equal(a[2], b[2]) and all(np.array_equal(a[0][q, :a[2][q]], b[0][q, :b[2][q]]) for q in range(B)))
    return {"shardset_call": new, "host_calls_plus_numpy_merge": old, "same_answer": same}


def shard_set(storage):
    shards = []
    for s in range(S):
        lo, hi = shard_range(n, S, s)
        ix = ca.HNSWIndex(d, ca.HNSWHyperParams(), ca.DistanceMetric.Cosine, storage, (-1.0, 1.0), id_base=lo)
        shards.append(ix.upload_vectors(np.ascontiguousarray(X[lo:hi])))
    return shards, ShardSet(shards)


results = {}
shards, ss = shard_set(ca.StorageType.UnsignedByte())
for k in (10, 512):
    results[f"bruteforce k {k}"] = pair(lambda: ss.bruteforce_topk(Q, k), lambda: [sh.bruteforce_topk(Q, k) + (np.full(B, k),) for sh in shards], k)
for k in (10, 204):
    results[f"flat u8 top_k {k}"] = pair(lambda: ss.flat_search(Q, k), lambda: [sh.flat_search(Q, k) for sh in shards], k)
u = rng.random(n) < 0.1
results["flat u8 top_k 10, 10 % of the rows live"] = pair(
    lambda: ss.flat_search(Q, 10, masks=u),
    lambda: [sh.flat_search_masked(Q, 10, u[slice(*shard_range(n, S, s))]) for s, sh in enumerate(shards)], 10)
ss.close()
for sh in shards:
    sh.close()

if args.filtered_n:
    from tests import meta_helpers as MH
    m = args.filtered_n
    scs = [MH.Scenario(n=m, dim=64, seed=20 + s) for s in range(S)]
    fsh = []
    for s, sc in enumerate(scs):
        dix = sc.device_index(id_base=s * m * MH.REPLICAS)
        dix.build(256)
        dix.build_meta(sc.node_ids, sc.mbits, sc.max_levels, 256)
        fsh.append(dix)
    fq, off, rows, _ = scs[0].queries(nq=B, seed=5)
    rows8 = rows.astype(np.int8)
    fss = ShardSet(fsh)
    new, a = timed(lambda: fss.search_filtered(fq, off, rows8, 10))
    old, b = timed(lambda: host_merge([sh.search_filtered(fq, off, rows8, 10) for sh in fsh], 10))
    results[f"filtered top_k 10, {S} x {m} embeddings of 64 dims"] = {
        "shardset_call": new, "host_calls_plus_numpy_merge": old,
        "same_answer": bool(np.array_equal(a[2], b[2]) and all(np.array_equal(a[0][q, :a[2][q]], b[0][q, :b[2][q]]) for q in range(B)))}
    fss.close()

# the wide merge alone: S lists of k keys per query, every list full
dev = torch.device("cuda:0")
merge = {}
for Sm, k in ((8, 128), (8, 256), (8, 512), (16, 512)):
    r = np.random.default_rng(Sm * k)
    ids = r.permutation(Sm * B * k).astype(np.uint32).reshape(Sm, B * k)
    sc = -np.sort(-r.random((Sm, B, k)).astype(np.float32), axis=2).reshape(Sm, B * k)
    rec = torch.from_numpy(np.ascontiguousarray(np.concatenate([ids.view(np.int32), sc.view(np.int32), np.full((Sm, B), k, np.int32)], axis=1))).to(dev)
    o_i = torch.zeros(B, k, dtype=torch.int32, device=dev); o_s = torch.zeros(B, k, device=dev); o_c = torch.zeros(B, dtype=torch.int32, device=dev)
    for _ in range(3):
        merge_lists_packed_device(rec, B, k, o_i, o_s, o_c, 0, 0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    e0.record()
    for _ in range(reps):
        merge_lists_packed_device(rec, B, k, o_i, o_s, o_c, 0, 0)
    e1.record()
    torch.cuda.synchronize()
    merge[f"{Sm} x {k} = {Sm * k} keys"] = {"us_per_launch": e0.elapsed_time(e1) * 1e3 / reps}
results["merge alone, 256 queries"] = merge

print(json.dumps({"config": {"workload": f"{S} shards of {n} x {d} clustered vectors on one device, {B}-query calls, 2 warm-up + {args.reps} timed calls per case",
                             "library": _lib.SO_PATH}, "cases": results}))
