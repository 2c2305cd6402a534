#!/usr/bin/env python3
"""The pair walk (kernels_walk_pair.hip; tuning knobs walk_pair, walk_pair_cache) on ONE index: ms per 32768-query launch with two
launches in flight (as bench.py runs them), the lower range's time in a launch that runs alone, and the pair kernel's counters
(cos_index_last_pair_stats: cache hits and code rows fetched below the cut), for every variant in PROBE_VARIANTS, the variants
ALTERNATING for PROBE_ROUNDS rounds so that drift hits all of them alike.  PROBE_SHAPE = c4shard (12.5M x 1024, M0 256 / M 64,
ef 112: the flagship) or c2 (1M x 768, M0 64 / M 32, ef 64); PROBE_N / PROBE_EF override.  One JSON line per variant; ids, scores and
counts must not change between variants."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
import cosdata_amd as ca  # noqa: E402
from cosdata_amd import _lib  # noqa: E402

SHAPES = {"c4shard": (12_500_000, 1024, 256, 64, 256, 112), "c2": (1_000_000, 768, 64, 32, 128, 64)}
SHAPE = os.environ.get("PROBE_SHAPE", "c4shard")
N, D, M0, M, EFC, EF = SHAPES[SHAPE]
N = int(os.environ.get("PROBE_N", N))
EF = int(os.environ.get("PROBE_EF", EF))
ROUNDS = int(os.environ.get("PROBE_ROUNDS", 3))
REPS = int(os.environ.get("PROBE_REPS", 12))
VARIANTS = [v for v in os.environ.get("PROBE_VARIANTS", "walk_pair=0;walk_pair=1,walk_pair_cache=256;walk_pair=1,walk_pair_cache=512;"
                                      "walk_pair=1,walk_pair_cache=1024").split(";") if v]
B, K = 32768, 10
dev = torch.device("cuda:0")
gc = torch.Generator(device=dev)
gc.manual_seed(4242)
centers = torch.randn(max(64, N // 1000), D, generator=gc, device=dev)
centers /= centers.norm(dim=1, keepdim=True)
X = bench.mixture(torch, N, D, 42, dev, centers)
Q = bench.mixture(torch, 2 * B, D, 43, dev, centers)
vr = ca.sample_values_range(X[:1000].cpu().numpy(), 1.0)
hp = ca.HNSWHyperParams(num_layers=9, ef_construction=EFC, ef_search=EF, level_0_neighbors_count=M0, neighbors_count=M)
ix = ca.HNSWIndex(D, hp, ca.DistanceMetric.Cosine, ca.StorageType.UnsignedByte(), vr, shortlist_size=64, device=0, seed=42)
ix.upload_vectors_device(X.data_ptr(), N, keepalive=X)
t0 = time.time()
ix.build(4096)
build_s = time.time() - t0
out = [tuple(torch.zeros(*s, dtype=t, device=dev) for s, t in (((B, K), torch.int32), ((B, K), torch.float32), ((B,), torch.int32), ((B,), torch.int32)))
       for _ in range(2)]
streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
ix.enable_timing(True)
print(json.dumps({"shape": SHAPE, "n": N, "dim": D, "m0": M0, "m": M, "ef": EF, "build_s": round(build_s, 2), "cut_after_levels": ix.walk_order_cuts(),
                  "table": ix.walk_table_info(), "level_counts": [ix.level_count(l) for l in range(10)]}), flush=True)


def launch(i, s):
    q = Q[(i % 2) * B:(i % 2 + 1) * B]
    o = out[s]
    ix.batch_search_device(q.data_ptr(), B, K, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), streams[s].cuda_stream)


def run(in_flight, reps):
    for i in range(4):
        launch(i, i % in_flight)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(reps):
        launch(i, i % in_flight)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


def set_variant(variant):
    _lib.tuning_clear(None)
    for kv in variant.split(","):
        k, v = kv.split("=")
        _lib.tuning_set(k.strip(), int(v))


res = {v: {"ms2": [], "lower_ms": []} for v in VARIANTS}
ref = None
for r in range(ROUNDS):
    for v in VARIANTS:
        set_variant(v)
        run(1, 2)
        sp = ix.last_walk_split(streams[0].cuda_stream)
        ps = ix.last_pair_stats(streams[0].cuda_stream)
        res[v]["lower_ms"].append(round(sp.lower_ms, 4))
        res[v]["upper_ms"] = round(sp.upper_ms, 4)
        res[v]["lower_evals"], res[v]["cache_entries"], res[v]["cache_hits"], res[v]["row_evals"] = sp.lower_evals, ps.cache_entries, ps.cache_hits, ps.row_evals
        res[v]["ms2"].append(round(run(2, REPS), 4))
        got = [torch.cat([out[0][j], out[1][j]]).clone() for j in range(4)]
        same = True if ref is None else all(bool(torch.equal(a, b)) for a, b in zip(got, ref))
        ref = got if ref is None else ref
        res[v]["outputs_identical_to_first_variant"] = res[v].get("outputs_identical_to_first_variant", True) and same
        res[v]["failed_queries"] = int((got[3] != 0).sum().item())
for v in VARIANTS:
    d = res[v]
    probed = d["cache_hits"] + d["row_evals"]
    print(json.dumps({"variant": v, "ms_per_launch_2_in_flight": d["ms2"], "median_ms": round(statistics.median(d["ms2"]), 4),
                      "spread_ms": round(max(d["ms2"]) - min(d["ms2"]), 4), "qps_median": round(B / statistics.median(d["ms2"]) * 1e3),
                      "alone_lower_ms": d["lower_ms"], "alone_upper_ms": d["upper_ms"], "lower_evals": d["lower_evals"], "cache_entries": d["cache_entries"],
                      "cache_hits": d["cache_hits"], "row_evals": d["row_evals"], "hits_per_evaluation": round(d["cache_hits"] / probed, 4) if probed else 0.0,
                      "failed_queries": d["failed_queries"], "outputs_identical_to_first_variant": d["outputs_identical_to_first_variant"]}), flush=True)
