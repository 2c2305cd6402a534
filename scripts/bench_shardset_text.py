#!/usr/bin/env python3
"""The text half of a shard set: c5's text collection (1M documents, Zipf vocabulary of 200k terms, 256 queries of 2-8
terms, top_k 30), everything on ONE device.  Three measurements, one JSON line:

  single   cos_bm25_search_batch_device on one handle of the whole collection, this build and (--parent-lib) the parent's build
           alternated in one process: the single-handle path did not move (its scoring kernels are the instructions they were);
  sharded  cos_shardset_bm25_search_batch over S = 1, 2, 8 id-range shards of the same collection against cos_bm25_search_batch on the
           one handle (host arrays in, host arrays out, wall clock), the same bits asserted; the exchange's data movement (S device
           copies of B x 4 KB) timed alone with HIP events, first loop dropped.  The fold kernel is NOT timed on its own here (that
           takes a kernel trace, which this script does not drive);
  hybrid   cos_shardset_hybrid_search_batch at S = 1 against cos_hybrid_search_batch on the same two indexes (--dense-n vectors of
           --dim dimensions built on the device): what going through the set costs.

    timeout -k 10 900 python scripts/bench_shardset_text.py [--parent-lib PATH]

One device runs its shards' scoring kernels one after the other, so nothing here shows what S GPUs gain by scoring at once."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--docs", type=int, default=1_000_000)
ap.add_argument("--vocab", type=int, default=200_000)
ap.add_argument("--doc-len", type=float, default=120.0)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--top-k", type=int, default=30)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--dense-n", type=int, default=100_000)
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--parent-lib", default=None)
a = ap.parse_args()

import torch
import cosdata_amd as ca
from cosdata_amd import _lib
from cosdata_amd.shardset import ShardSet
from bench_bm25_update import Raw, csr_of, spread, text_corpus

dev = torch.device("cuda:0")
n, V, B, k = a.docs, a.vocab, a.batch, a.top_k
hashes, p_term, p_doc, tf, pz = text_corpus(torch, dev, n, V, a.doc_len)
whole_csr = csr_of(torch, V, hashes, p_term, p_doc, tf)
rng = np.random.default_rng(5)
th_all, pz_h = hashes.cpu().numpy().astype(np.uint32), pz.cpu().numpy()
qt, qo = [], [0]
for _ in range(B):                                                                   # bench_c5's queries: 2-8 terms, Zipf-distributed
    m = int(rng.integers(2, 9))
    qt.append(th_all[rng.choice(V, m, replace=False, p=pz_h)]); qo.append(qo[-1] + m)
qt, qo = np.concatenate(qt).astype(np.uint32), np.array(qo, np.uint32)


def shard_csrs(S):
    out, bounds = [], [n * s // S for s in range(S + 1)]
    for s in range(S):
        c = csr_of(torch, V, hashes, p_term, p_doc, tf, (p_doc >= bounds[s]) & (p_doc < bounds[s + 1]))
        out.append((c[0], c[1], (c[2] - np.uint32(bounds[s])).astype(np.uint32), c[3]))
    return out, bounds


def stubs(bounds):
    X = np.random.default_rng(1).standard_normal((4, 8)).astype(np.float32)
    return [ca.HNSWIndex(8, ca.HNSWHyperParams(num_layers=3), id_base=int(b)).upload_vectors(X) for b in bounds[:-1]]


def wall(call, reps):
    call(); call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = call(); ts.append((time.perf_counter() - t) * 1e3)
    return spread(ts), out


def same(x, y):
    return bool(np.array_equal(x[2], y[2]) and all(np.array_equal(x[0][q, :x[2][q]], y[0][q, :y[2][q]]) and
                                                    np.array_equal(x[1][q, :x[2][q]].view(np.uint32), y[1][q, :y[2][q]].view(np.uint32)) for q in range(B)))


out = {"bench": "shardset_text", "docs": n, "vocab": V, "postings": int(whole_csr[2].size), "batch": B, "top_k": k, "library": _lib.SO_PATH}

# ---- 1. the single-handle path, parent build and this build alternated ----
st = torch.cuda.Stream(device=dev)
o_i = torch.zeros(B, k, dtype=torch.int32, device=dev); o_s = torch.zeros(B, k, device=dev); o_c = torch.zeros(B, dtype=torch.int32, device=dev)


def timed_device(lib, h):
    lib.search_device(h, qt, qo, k, o_i, o_s, o_c, st.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(a.reps):
        lib.search_device(h, qt, qo, k, o_i, o_s, o_c, st.cuda_stream)
    e1.record(st); st.synchronize()
    return e0.elapsed_time(e1) / a.reps


new = Raw(_lib.SO_PATH)
par = Raw(a.parent_lib) if a.parent_lib else None
h_new = new.create(whole_csr, n)
h_par = par.create(whole_csr, n) if par else None
ms = {"parent": [], "tree": []}
for _ in range(a.rounds):
    if par:
        ms["parent"].append(timed_device(par, h_par))
    ms["tree"].append(timed_device(new, h_new))
out["single_handle_ms_per_batch"] = {key: spread(v) for key, v in ms.items() if v}
if par:
    par.destroy(h_par)
new.destroy(h_new)

# ---- 2. the sharded call against one handle ----
whole = ca.BM25Index(*whole_csr, n)
one, ref = wall(lambda: whole.search_batch(qt, qo, k), a.reps)
out["one_handle_host_call_ms"] = one
out["sharded"] = {}
for S in (1, 2, 8):
    csrs, bounds = shard_csrs(S)
    bm = [ca.BM25Index(*c, bounds[s + 1] - bounds[s]) for s, c in enumerate(csrs)]
    ss = ShardSet(stubs(bounds)).attach_bm25(bm)
    t, got = wall(lambda: ss.bm25_search(qt, qo, k), a.reps)
    src = [torch.zeros(B * 512, dtype=torch.int64, device=dev) for _ in range(S)]      # the exchange's data movement alone
    dst = torch.zeros(S, B * 512, dtype=torch.int64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ex = []
    for r in range(1 + a.rounds):                                                      # the first loop warms up and is dropped
        e0.record()
        for _ in range(a.reps):
            for s in range(S):
                dst[s].copy_(src[s], non_blocking=True)
        e1.record(); torch.cuda.synchronize()
        if r:
            ex.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    out["sharded"][f"S={S}"] = {"set_call_ms": t, "same_bits_as_one_handle": same(got, ref), "exchange_copies_us_per_call": spread(ex),
                                "exchange_bytes": S * B * 4096}
    ss.close()
    del bm

# ---- 3. hybrid through the set at S = 1 against the single-index call ----
if a.dense_n:
    r = np.random.default_rng(7)
    centers = r.uniform(-0.8, 0.8, (64, a.dim)).astype(np.float32)
    X = np.clip(centers[r.integers(0, 64, a.dense_n)] + 0.2 * r.standard_normal((a.dense_n, a.dim)).astype(np.float32), -0.999, 0.999).astype(np.float32)
    Q = np.clip(centers[r.integers(0, 64, B)] + 0.2 * r.standard_normal((B, a.dim)).astype(np.float32), -0.999, 0.999).astype(np.float32)
    ix = ca.HNSWIndex(a.dim, ca.HNSWHyperParams(), ca.DistanceMetric.Cosine, ca.StorageType.UnsignedByte(), (-1.0, 1.0))
    ix.upload_vectors(X).build(4096)
    hk = 10
    direct, d_out = wall(lambda: ca.hybrid_search_batch(ix, whole, Q, qt, qo, hk), a.reps)
    ss = ShardSet([ix]).attach_bm25([whole], np.zeros(1, np.uint32))
    via, s_out = wall(lambda: ss.hybrid_search(Q, qt, qo, hk), a.reps)
    direct2, _ = wall(lambda: ca.hybrid_search_batch(ix, whole, Q, qt, qo, hk), a.reps)
    out["hybrid_S1"] = {"dense": f"{a.dense_n} x {a.dim} u8", "top_k": hk, "cos_hybrid_search_batch_ms": direct, "cos_shardset_hybrid_search_batch_ms": via,
                        "cos_hybrid_search_batch_again_ms": direct2, "same_bits": same(s_out, d_out)}
    ss.close()
print(json.dumps(out))
