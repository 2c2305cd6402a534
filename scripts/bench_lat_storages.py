#!/usr/bin/env python3
"""Small launches over f16 / f32 rows and binary / octal codes: the throughput kernel (what these storages got before the latency
kernels took them: cos_index_set_latency_mode(0)) against the one-wave and the four-wave latency kernel, on one device-built index
per storage.  Per (storage, launch size, ef): two warm-up calls per kernel, then `--reps` rounds that ALTERNATE the three kernels;
the median and the spread (min .. max) of the walk's HIP-event time (cos_search_stats.walk_ms) and of the call's wall time.  Every
timed answer is compared with the throughput kernel's (ids, score bits, counts).  One JSON line per storage, as it completes; exit
status 1 on any mismatch.

    timeout -k 10 900 python scripts/bench_lat_storages.py --out results.jsonl
    timeout -k 10 900 python scripts/bench_lat_storages.py --lib /path/to/another/libcosdata_hip.so --kernels throughput

The second form times another build of the library (the parent commit's) on the same corpus and graph."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--storages", nargs="*", default=["f16", "binary", "f32", "octal"])
ap.add_argument("--batches", type=int, nargs="*", default=[256, 2048])
ap.add_argument("--efs", type=int, nargs="*", default=[64, 256])
ap.add_argument("--kernels", nargs="*", default=["throughput", "latency", "latency_waves"])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--build-batch", type=int, default=4096)
ap.add_argument("--deadline", type=float, default=1e9, help="seconds after which no further storage is started")
ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
ap.add_argument("--lib", default=None, help="load this libcosdata_hip.so instead of the tree's")
args = ap.parse_args()

from cosdata_amd import _lib
if args.lib:
    _lib.SO_PATH = os.path.abspath(args.lib)
import cosdata_amd as ca

t_start = time.perf_counter()
n, d = args.n, args.dim
rng = np.random.default_rng(42)
nc = max(64, n // 1000)
centers = rng.uniform(-0.8, 0.8, (nc, d)).astype(np.float32)
X = np.empty((n, d), np.float32)
for s in range(0, n, 1 << 16):
    k = min(1 << 16, n - s)
    X[s:s + k] = np.clip(centers[rng.integers(0, nc, k)] + 0.2 * rng.standard_normal((k, d), dtype=np.float32), -0.999, 0.999)
Q = np.clip(X[rng.integers(0, n, max(args.batches))] + 0.02 * rng.standard_normal((max(args.batches), d), dtype=np.float32), -0.999, 0.999)

KINDS = {"f16": ca.StorageType(ca.StorageKind(2), 0), "f32": ca.StorageType(ca.StorageKind(3), 0),
         "binary": ca.StorageType.SubByte(1), "octal": ca.StorageType.SubByte(3)}
SETTINGS = {"throughput": (0, 0), "latency": (0xFFFFFFFF, 0), "latency_waves": (0xFFFFFFFF, 0xFFFFFFFF)}
bad_total = 0
for name in args.storages:
    if time.perf_counter() - t_start > args.deadline:
        print(f"deadline: {name} not started", file=sys.stderr)
        continue
    hp = ca.HNSWHyperParams(ef_construction=64, ef_search=64)
    ix = ca.HNSWIndex(d, hp, ca.DistanceMetric.Cosine, KINDS[name], (-1.0, 1.0))
    t = time.perf_counter()
    ix.upload_vectors(X).build(args.build_batch)
    build_s = time.perf_counter() - t
    ix.enable_timing(True)
    cases = {}
    for ef in args.efs:
        ix.set_ef_search(ef)
        for B in args.batches:
            q = Q[:B]
            ran, walk, wall, ref = {}, {k: [] for k in args.kernels}, {k: [] for k in args.kernels}, None

            def call(kernel):
                ix.set_latency_mode(SETTINGS[kernel][0])
                ix.set_latency_waves(SETTINGS[kernel][1])
                t0 = time.perf_counter()
                out = ix.batch_search(q, 10)
                return out, (time.perf_counter() - t0) * 1e3

            for k in args.kernels:
                call(k); call(k)
            for _ in range(args.reps):
                for k in args.kernels:
                    out, ms = call(k)
                    wall[k].append(ms)
                    walk[k].append(float(ix.last_stats().walk_ms))
                    if hasattr(ix, "last_walk_kernel"):
                        ran[k] = ix.last_walk_kernel()
                    if ref is None:
                        ref = out
                    elif not (np.array_equal(out[0], ref[0]) and np.array_equal(out[1].view(np.uint32), ref[1].view(np.uint32)) and np.array_equal(out[2], ref[2])):
                        bad_total += 1
            cases[f"B {B} ef {ef}"] = {k: {"kernel_ran": ran.get(k), "walk_ms_median": round(float(np.median(walk[k])), 4),
                                           "walk_ms_min": round(min(walk[k]), 4), "walk_ms_max": round(max(walk[k]), 4),
                                           "call_ms_median": round(float(np.median(wall[k])), 4)} for k in args.kernels}
    line = json.dumps({"storage": name, "workload": f"{n} x {d} clustered vectors, device-built graph (ef_construction 64), 2 warm-up + {args.reps} alternating timed calls",
                       "library": _lib.SO_PATH, "build_s": round(build_s, 1), "cases": cases, "mismatching_answers": bad_total})
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    del ix
sys.exit(1 if bad_total else 0)
