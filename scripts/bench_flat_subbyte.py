#!/usr/bin/env python3
"""The exhaustive scan over the bit-plane storages: cos_flat_search_batch at top_k 10 over a binary, a quaternary and an octal index
(and a u8 one on request) of one clustered corpus, at 768 and 1024 dims, under the default kernels, `flat_fp4 = 0` (i8 digits in the
query-resident kernel) and `flat_tile_kernel = 1` (the 256 x 128 tile kernel).  256-query calls; per case two warm-up calls (the first
sizes the workspace) and `--reps` timed ones: the median wall time of a call, the median HIP-event time of its scan kernels
(cos_flat_stats.gemm_ms), and the scan kernels' rate int8_ops / gemm_ms as a share of the matrix peak of the digit format that ran
(e2m1 on the scaled MFMA: 10 PF; i8: 5 PF) next to the streamed code bytes per second.  The default answer of every case is compared
with the oracle's on a sample of the queries (ids, score bits, counts), and the knobs' answers with the default's.  One JSON line; exit
status 1 on any mismatch.

    timeout -k 10 900 python scripts/bench_flat_subbyte.py
    timeout -k 10 300 python scripts/bench_flat_subbyte.py --storages quaternary u8 --no-parity --lib /path/to/another/libcosdata_hip.so

The second form times another build of the library (the parent commit's, say) on the same corpus: run the two alternately."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4_000_000)
ap.add_argument("--dims", type=int, nargs="*", default=[768, 1024])
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--top-k", type=int, default=10)
ap.add_argument("--storages", nargs="*", default=["binary", "quaternary", "octal"])
ap.add_argument("--knobs", nargs="*", default=["default", "flat_fp4=0", "flat_tile_kernel=1"])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sample", type=int, default=2, help="queries checked against the oracle")
ap.add_argument("--no-parity", action="store_true")
ap.add_argument("--lib", default=None, help="load this libcosdata_hip.so instead of the tree's")
args = ap.parse_args()

import torch
from cosdata_amd import _lib
if args.lib:
    _lib.SO_PATH = os.path.abspath(args.lib)
import cosdata_amd as ca
from oracle import oracle as O

PEAK_I8, PEAK_FP4 = 5.0e15, 10.0e15                  # dense matrix peaks of the part, operations per second
KINDS = {"binary": (ca.StorageType.SubByte(1), O.STORAGE_SUBBYTE, 1), "quaternary": (ca.StorageType.SubByte(2), O.STORAGE_SUBBYTE, 2),
         "octal": (ca.StorageType.SubByte(3), O.STORAGE_SUBBYTE, 3), "u8": (ca.StorageType.UnsignedByte(), O.STORAGE_U8, 0)}
n, B, k = args.n, args.batch, args.top_k
dev = torch.device("cuda:0")
sample = np.linspace(0, B - 1, min(args.sample, B)).astype(int)


def corpus(d):
    g = torch.Generator(device=dev); g.manual_seed(7)
    nc = max(64, n // 1000)
    centers = torch.rand(nc, d, generator=g, device=dev) * 1.6 - 0.8

    def draw(m, seed):
        gg = torch.Generator(device=dev); gg.manual_seed(seed)
        out = torch.empty(m, d, device=dev)
        for s in range(0, m, 1 << 18):
            c = min(1 << 18, m - s)
            idx = torch.randint(0, nc, (c,), generator=gg, device=dev)
            out[s:s + c] = (centers[idx] + 0.2 * torch.randn(c, d, generator=gg, device=dev)).clamp_(-0.999, 0.999)
        return out
    return draw(n, 42), draw(B, 43).cpu().numpy()


def timed(call):
    call(); call()
    wall, gemm, out = [], [], None
    for _ in range(args.reps):
        t = time.perf_counter()
        out = call()                                  # returns after the call's last copy back: the stream is drained
        wall.append((time.perf_counter() - t) * 1e3)
        gemm.append(out[3].gemm_ms)
    return out, float(np.median(wall)), float(np.median(gemm)), wall


def same(a, b):
    return np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


results, bad_total = {}, 0
for d in args.dims:
    X, Qh = corpus(d)
    torch.cuda.synchronize()
    Xh = None if args.no_parity else X.cpu().numpy()
    for name in args.storages:
        st_dev, st_o, res = KINDS[name]
        ix = ca.HNSWIndex(d, ca.HNSWHyperParams(), ca.DistanceMetric.Cosine, st_dev, (-1.0, 1.0))
        ix.upload_vectors_device(X.data_ptr(), n, keepalive=X)
        ref = None
        for knob in args.knobs:
            kw = {} if knob == "default" else {knob.split("=")[0]: int(knob.split("=")[1])}
            with _lib.tuning(**kw):
                out, wall, gemm, walls = timed(lambda: ix.flat_search(Qh, k, with_stats=True))
            st = out[3]
            fp4 = name in ("binary", "quaternary") and "flat_fp4" not in kw and "flat_tile_kernel" not in kw
            rate = st.int8_ops / (gemm * 1e-3)
            r = {"ms_per_call": wall, "scan_kernels_ms": gemm, "scan_launches": int(st.gemm_launches), "digit_ops": st.int8_ops,
                 "digit_format": "e2m1" if fp4 else "i8", "scan_pops": rate / 1e15, "share_of_matrix_peak": rate / (PEAK_FP4 if fp4 else PEAK_I8),
                 "code_tb_per_s": st.code_bytes / (gemm * 1e-3) / 1e12, "ms_all": [round(x, 4) for x in walls]}
            if ref is None:
                ref = out
                if Xh is not None:
                    oix = O.OracleIndex(O.HNSWParams(dim=d, storage=st_o, resolution=res, range_lo=-1.0, range_hi=1.0)).set_vectors(Xh)
                    oi, os_, oc = oix.flat_search_batch(Qh[sample], k, threads=16)
                    del oix
                    bad = sum(not (int(out[2][b]) == int(oc[j]) and np.array_equal(out[0][b], oi[j]) and
                                   np.array_equal(out[1][b].view(np.uint32), os_[j].view(np.uint32))) for j, b in enumerate(sample))
                    r["mismatching_sampled_queries"] = int(bad)
                    bad_total += bad
            else:
                r["equals_default"] = bool(same(out, ref))
                bad_total += not r["equals_default"]
            results[f"{n} x {d} {name} {knob}"] = r
        del ix
    del X, Xh

print(json.dumps({"config": {"workload": f"{n} clustered vectors, {B}-query calls at top_k {k}, 2 warm-up + {args.reps} timed calls per case (median)",
                             "library": _lib.SO_PATH, "parity_sample": None if args.no_parity else len(sample)},
                  "cases": results, "mismatches": int(bad_total)}))
sys.exit(1 if bad_total else 0)
