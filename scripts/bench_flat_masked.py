#!/usr/bin/env python3
"""What a row mask costs the exhaustive code scan: cos_flat_search_masked_batch over a quaternary and a u8 index of one clustered
768-dim corpus, 256-query calls, top_k 10.  Cases per storage: the unmasked call; an all-ones mask; masks with 90 %, 50 % and 1 % of
the rows live; 1 % of the rows in the handle's deleted set (COS_SCAN_SKIP_DELETED, no allow-list); four masks mixed per query; and the
1 % mask on the score-matrix path (tuning knob flat_unfused = 1) for comparison.  Per case two warm-up calls and `--reps` timed ones:
median and min-max wall time of a call and the median HIP-event time of its scan kernels.  One JSON line.

    timeout -k 10 600 python scripts/bench_flat_masked.py

The deleted set is filled through cos_index_delete, which needs a built graph: `--delete-n` rows (default 20 000, a corpus of its
own) are built and 1 % of them deleted to time that case at that size; at the big corpus the same bitmap is timed as an allow-list
(the kernels see one effective mask either way: allow-list AND NOT deleted)."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--top-k", type=int, default=10)
ap.add_argument("--storages", nargs="*", default=["quaternary", "u8"])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--delete-n", type=int, default=20_000)
args = ap.parse_args()

import torch
from cosdata_amd import _lib
import cosdata_amd as ca
from cosdata_amd.index import pack_row_masks

n, d, B, K = args.n, args.dim, args.batch, args.top_k
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
rng = np.random.default_rng(5)
u = rng.random(n)
packed = {name: pack_row_masks(m) for name, m in (("all ones", np.ones(n, bool)), ("90 % live", u < 0.9), ("50 % live", u < 0.5), ("1 % live", u < 0.01),
                                                  ("99 % live (the 1 % deleted bitmap as an allow-list)", u >= 0.01))}
four = np.ascontiguousarray(np.concatenate([packed["90 % live"], packed["50 % live"], packed["1 % live"], packed["all ones"]]))
qm4 = (np.arange(B) % 4).astype(np.uint32)


def timed(call):
    call(); call()
    wall, gemm = [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t) * 1e3)
        gemm.append(out[3].gemm_ms)
    return {"ms_per_call": float(np.median(wall)), "ms_min": float(min(wall)), "ms_max": float(max(wall)), "scan_kernels_ms": float(np.median(gemm)),
            "scan_launches": int(out[3].gemm_launches), "full_lists": int((out[2] == K).sum())}


KINDS = {"quaternary": ca.StorageType.SubByte(2), "u8": ca.StorageType.UnsignedByte()}
results = {}
for name in args.storages:
    ix = ca.HNSWIndex(d, ca.HNSWHyperParams(), ca.DistanceMetric.Cosine, KINDS[name], (-1.0, 1.0))
    ix.upload_vectors_device(X.data_ptr(), n, keepalive=X)
    r = {"unmasked": timed(lambda: ix.flat_search(Qh, K, with_stats=True))}
    for case, bits in packed.items():
        r[case] = timed(lambda: ix.flat_search_masked(Qh, K, bits, with_stats=True))
    r["4 masks mixed per query"] = timed(lambda: ix.flat_search_masked(Qh, K, four, qm4, with_stats=True))
    with _lib.tuning(flat_unfused=1):
        r["1 % live, flat_unfused = 1"] = timed(lambda: ix.flat_search_masked(Qh, K, packed["1 % live"], with_stats=True))
        r["unmasked, flat_unfused = 1"] = timed(lambda: ix.flat_search(Qh, K, with_stats=True))
    r["unmasked again"] = timed(lambda: ix.flat_search(Qh, K, with_stats=True))
    ix.close()
    # the deleted set proper, at the size a graph is built in seconds
    m = min(args.delete_n, n)
    small = ca.HNSWIndex(d, ca.HNSWHyperParams(num_layers=3, ef_construction=32, ef_search=32), ca.DistanceMetric.Cosine, KINDS[name], (-1.0, 1.0))
    small.upload_vectors(X[:m].cpu().numpy()).build(1024)
    r[f"{m} rows: unmasked"] = timed(lambda: small.flat_search(Qh, K, with_stats=True))
    small.delete(rng.permutation(m)[:max(1, m // 100)].astype(np.uint32))
    r[f"{m} rows: 1 % deleted, skip_deleted"] = timed(lambda: small.flat_search_masked(Qh, K, skip_deleted=True, with_stats=True))
    r[f"{m} rows: deleted_count"] = small.deleted_count()
    small.close()
    results[name] = r

print(json.dumps({"config": {"workload": f"{n} x {d} clustered vectors, {B}-query calls, top_k {K}, 2 warm-up + {args.reps} timed calls per case",
                             "library": _lib.SO_PATH}, "cases": results}))
