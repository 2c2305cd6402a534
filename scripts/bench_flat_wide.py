#!/usr/bin/env python3
"""The exhaustive scans at every survivor-pool width: cos_flat_search_batch at top_k 10 .. 204 (pools of 64 .. 1024 keys) over a
quaternary and a u8 index of one clustered 768-dim corpus, and cos_bruteforce_topk at k 10 .. 512 over its raw rows.  256-query
calls; per case two warm-up calls (the first sizes the workspace) and `--reps` timed ones: the median wall time of a call, the
median HIP-event time of its scan kernels (cos_flat_stats.gemm_ms) and the difference — selection, append folds, rerank, copies and
host work.  Every timed answer is compared with the oracle's on a sample of the queries (ids, score bits, counts).  One JSON line;
exit status 1 on any mismatch.

    timeout -k 10 900 python scripts/bench_flat_wide.py
    timeout -k 10 300 python scripts/bench_flat_wide.py --flat-k 10 --brute-k --no-parity --lib /path/to/another/libcosdata_hip.so

The second form times another build of the library (the parent commit's, say) on the same corpus: run the two alternately."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=2_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--flat-k", type=int, nargs="*", default=[10, 12, 13, 25, 51, 102, 204])
ap.add_argument("--brute-k", type=int, nargs="*", default=[10, 32, 100, 512])
ap.add_argument("--storages", nargs="*", default=["quaternary", "u8"])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sample", type=int, default=4, help="queries checked against the oracle")
ap.add_argument("--no-parity", action="store_true")
ap.add_argument("--lib", default=None, help="load this libcosdata_hip.so instead of the tree's")
args = ap.parse_args()

import torch
from cosdata_amd import _lib
if args.lib:
    _lib.SO_PATH = os.path.abspath(args.lib)
import cosdata_amd as ca
from oracle import oracle as O

n, d, B = args.n, args.dim, args.batch
dev = torch.device("cuda:0")
g = torch.Generator(device=dev); g.manual_seed(7)
nc = max(64, n // 1000)
centers = torch.rand(nc, d, generator=g, device=dev) * 1.6 - 0.8


def draw(m, seed):
    gg = torch.Generator(device=dev); gg.manual_seed(seed)
    out = torch.empty(m, d, device=dev)
    for s in range(0, m, 1 << 18):
        k = min(1 << 18, m - s)
        idx = torch.randint(0, nc, (k,), generator=gg, device=dev)
        out[s:s + k] = (centers[idx] + 0.2 * torch.randn(k, d, generator=gg, device=dev)).clamp_(-0.999, 0.999)
    return out


X = draw(n, 42)
Qh = draw(B, 43).cpu().numpy()
torch.cuda.synchronize()
sample = np.linspace(0, B - 1, min(args.sample, B)).astype(int)
Xh = None if args.no_parity else X.cpu().numpy()


def pool_width(need):
    return next(p for p in (64, 128, 256, 512, 1024) if need <= p)


def timed(call):
    call(); call()
    wall, gemm, out = [], [], None
    for _ in range(args.reps):
        t = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t) * 1e3)
        gemm.append(out[3].gemm_ms if len(out) > 3 else float("nan"))
    return out, float(np.median(wall)), float(np.median(gemm)), wall


results, bad_total = {}, 0
KINDS = {"quaternary": (ca.StorageType.SubByte(2), O.STORAGE_SUBBYTE, 2), "u8": (ca.StorageType.UnsignedByte(), O.STORAGE_U8, 0)}
ix = None
for name in args.storages:
    st_dev, st_o, res = KINDS[name]
    ix = ca.HNSWIndex(d, ca.HNSWHyperParams(), ca.DistanceMetric.Cosine, st_dev, (-1.0, 1.0))
    ix.upload_vectors_device(X.data_ptr(), n, keepalive=X)
    oix = None if args.no_parity else O.OracleIndex(O.HNSWParams(dim=d, storage=st_o, resolution=res, range_lo=-1.0, range_hi=1.0)).set_vectors(Xh)
    for k in args.flat_k:
        out, wall, gemm, walls = timed(lambda: ix.flat_search(Qh, k, with_stats=True))
        r = {"pool": pool_width(5 * k), "ms_per_call": wall, "scan_kernels_ms": gemm, "selection_rerank_host_ms": wall - gemm,
             "scan_launches": int(out[3].gemm_launches), "ms_all": [round(x, 4) for x in walls]}
        if oix is not None:
            oi, os_, oc = oix.flat_search_batch(Qh[sample], k, threads=16)
            bad = 0
            for j, b in enumerate(sample):
                c = int(oc[j])
                bad += not (int(out[2][b]) == c and np.array_equal(out[0][b, :c], oi[j, :c])
                            and np.array_equal(out[1][b, :c].view(np.uint32), os_[j, :c].view(np.uint32)))
            r["mismatching_sampled_queries"] = int(bad)
            bad_total += bad
        results[f"flat {name} top_k {k}"] = r
    del oix

if args.brute_k:
    if ix is None:
        ix = ca.HNSWIndex(d, ca.HNSWHyperParams(), ca.DistanceMetric.Cosine, ca.StorageType.UnsignedByte(), (-1.0, 1.0))
        ix.upload_vectors_device(X.data_ptr(), n, keepalive=X)
    ref = None if args.no_parity else O.bruteforce_topk(Xh, Qh[sample], max(args.brute_k), threads=16)  # exact sort: a prefix is the smaller k's answer
    for k in args.brute_k:
        out, wall, _, walls = timed(lambda: ix.bruteforce_topk(Qh, k))
        r = {"pool": pool_width(2 * k), "ms_per_call": wall, "ms_all": [round(x, 4) for x in walls]}
        if ref is not None:
            bad = sum(not (np.array_equal(out[0][b], ref[0][j, :k]) and np.array_equal(out[1][b].view(np.uint32), ref[1][j, :k].view(np.uint32)))
                      for j, b in enumerate(sample))
            r["mismatching_sampled_queries"] = int(bad)
            bad_total += bad
        results[f"bruteforce k {k}"] = r

print(json.dumps({"config": {"workload": f"{n} x {d} clustered vectors, {B}-query calls, 2 warm-up + {args.reps} timed calls per case (median)",
                             "library": _lib.SO_PATH, "parity_sample": None if args.no_parity else len(sample)},
                  "cases": results, "mismatching_sampled_queries": None if args.no_parity else int(bad_total)}))
sys.exit(1 if bad_total else 0)
