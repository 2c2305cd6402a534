#!/usr/bin/env python3
"""Updates of the resident learned-sparse postings on scripts/bench_sparse.py's corpus (400 000 vectors x ~48 non-zeros over
30 000 dimensions, 6-bit keys; the same generator and the same 256-query batch), one JSON line:

  insert   the last 40 000 vectors into the 360 000-vector index (cos_sparse_insert) against the only way without it:
           cos_sparse_destroy + cos_sparse_create from the merged host CSR (the host-side merge is not even counted).  Same
           process, alternated, `--reps` repetitions each; medians and spread.
  delete   1 000 vectors per call (cos_sparse_delete) against the same destroy + create.
  search   kernel time (HIP events of cos_sparse_search_batch) of the 256-query batch on (b) a never-updated index, (c) the index
           that reached the same CSR through the insert, (d) after deleting 10 % of the vectors, against (e) a fresh create of the
           surviving CSR — and, with --parent-lib PATH (another build of libcosdata_hip.so, e.g. the parent commit's), (a) that
           build on the never-updated index, alternated with (b) round by round so that the spread of each against itself is known.

--profile-insert: one create + one insert + one delete and nothing else — the run to put under `rocprofv3 --kernel-trace --stats`
for postings_merge_kernel<SparseMerge<true>>'s (SparseMerge<false> in the unpacked layout) and sparse_compact_kernel's own time (bytes read + written per posting of the new array over that
time, against the streaming-copy ceiling cos_hbm_probe(kind = 1) reports on the same machine)."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

VOCAB, NNZ, BITS, UPPER, B, K = 30_000, 48, 6, 3.0, 256, 10


def corpus(torch, dev, n):
    """bench_sparse.py's generator -> the raw vectors as a CSR in id order (dims ascending inside a vector)"""
    g = torch.Generator(device=dev); g.manual_seed(3)
    pz = 1.0 / torch.arange(1, VOCAB + 1, device=dev, dtype=torch.float64) ** 0.9
    cdf = torch.cumsum(pz / pz.sum(), 0)
    dim = torch.searchsorted(cdf, torch.rand(n * NNZ, generator=g, device=dev, dtype=torch.float64)).clamp_(max=VOCAB - 1)
    vid = torch.arange(n, device=dev).repeat_interleave(NNZ)
    key_pair = torch.unique(dim * n + vid)                                   # one posting per (dim, vector)
    dim, vid = key_pair // n, key_pair % n
    val = torch.exp(0.6 * torch.randn(dim.numel(), generator=g, device=dev)).clamp_(max=UPPER * 1.2).float()
    o = torch.argsort(vid * VOCAB + dim)
    vid, dim, val = vid[o], dim[o], val[o]
    off = torch.searchsorted(vid, torch.arange(n + 1, device=dev))
    return (off.cpu().numpy().astype(np.uint64), dim.cpu().numpy().astype(np.uint32), val.cpu().numpy().astype(np.float32),
            (pz / pz.sum()).cpu().numpy())


def rows(raw, lo, hi):
    a, b = int(raw[0][lo]), int(raw[0][hi])
    return (raw[0][lo:hi + 1] - raw[0][lo]).astype(np.uint64), raw[1][a:b], raw[2][a:b]


def rows_of_ids(raw, ids):
    lo, hi = raw[0][ids].astype(np.int64), raw[0][ids + 1].astype(np.int64)
    off = np.zeros(ids.size + 1, np.uint64); off[1:] = np.cumsum(hi - lo)
    idx = np.concatenate([np.arange(x, y) for x, y in zip(lo, hi)])
    return off, raw[1][idx], raw[2][idx]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_float), ("blocks", C.c_uint32), ("postings_visited", C.c_uint64), ("posting_bytes", C.c_uint64)]


class Raw:
    """the learned-sparse entry points of ONE build of the library through plain ctypes (two builds can be loaded side by side)"""

    def __init__(self, path):
        self.L = C.CDLL(path)
        for name in ("cos_sparse_create", "cos_sparse_destroy", "cos_sparse_search_batch", "cos_sparse_last_stats", "cos_sparse_insert", "cos_sparse_delete",
                     "cos_sparse_download"):
            if hasattr(self.L, name):
                getattr(self.L, name).restype = C.c_int32
        self.L.cos_last_error_string.restype = C.c_char_p

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.L.cos_last_error_string().decode())

    @staticmethod
    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    def create(self, csr, n):
        h = C.c_void_p()
        self.ok(self.L.cos_sparse_create(C.c_int32(0), C.c_uint32(BITS), C.c_float(UPPER), self.p(csr[0]), C.c_uint32(csr[0].size), self.p(csr[1]), self.p(csr[2]),
                                         C.c_uint32(n), None, None, None, C.byref(h)))
        return h

    def destroy(self, h):
        self.ok(self.L.cos_sparse_destroy(h))

    def insert(self, h, u):
        self.ok(self.L.cos_sparse_insert(h, C.c_uint32(u[0].size - 1), self.p(u[0]), self.p(u[1]), self.p(u[2]), None))

    def delete(self, h, ids, u):
        removed = C.c_uint64(0)
        self.ok(self.L.cos_sparse_delete(h, self.p(ids), self.p(u[0]), C.c_uint32(ids.size), self.p(u[1]), self.p(u[2]), C.byref(removed)))
        return int(removed.value)

    def download(self, h):
        nt, nnz = C.c_uint32(0), C.c_uint64(0)
        self.ok(self.L.cos_sparse_download(h, C.byref(nt), C.byref(nnz), None, None, None))
        d, ko, vi = np.zeros(nt.value, np.uint32), np.zeros(nt.value * ((1 << BITS) + 1), np.uint64), np.zeros(max(int(nnz.value), 1), np.uint32)
        self.ok(self.L.cos_sparse_download(h, C.byref(nt), C.byref(nnz), self.p(d), self.p(ko), self.p(vi)))
        return d, ko, vi[:int(nnz.value)]

    def search(self, h, q, out):
        self.ok(self.L.cos_sparse_search_batch(h, self.p(q[0]), self.p(q[1]), self.p(q[2]), C.c_uint32(B), C.c_uint32(K), C.c_float(0.0), C.c_uint32(0),
                                               self.p(out[0]), self.p(out[1]), self.p(out[2])))
        st = Stats()
        self.ok(self.L.cos_sparse_last_stats(h, C.byref(st)))
        return st.kernel_ms


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=400_000)
    ap.add_argument("--grow", type=float, default=0.1, help="share of the vectors that arrives through cos_sparse_insert")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the search comparison")
    ap.add_argument("--search-reps", type=int, default=10, help="search calls per round (the round's figure is their median kernel time)")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--profile-insert", action="store_true")
    a = ap.parse_args()
    import torch
    import cosdata_amd as ca
    from cosdata_amd import _lib
    dev = torch.device("cuda:0")
    n = a.vectors
    n0 = n - int(n * a.grow)
    raw = corpus(torch, dev, n)
    pz_h = raw[3]
    torch.cuda.empty_cache()
    base = ca.sparse_build_csr(BITS, UPPER, *rows(raw, 0, n0))
    merged = ca.sparse_build_csr(BITS, UPPER, *rows(raw, 0, n))
    upd = rows(raw, n0, n)
    nnz, nnz_upd = int(merged[2].size), int(upd[1].size)
    new = Raw(_lib.SO_PATH)
    perm = np.random.default_rng(9).permutation(n)
    dele = lambda lo, hi: (np.sort(perm[lo:hi]).astype(np.uint32),) + (rows_of_ids(raw, np.sort(perm[lo:hi])),)
    if a.profile_insert:
        h = new.create(base, n0)
        packed = C.c_uint32(0)
        new.ok(new.L.cos_sparse_layout(h, C.byref(packed)))
        new.insert(h, upd)
        ids, u = dele(0, 1000)
        removed = new.delete(h, ids, u)
        new.destroy(h)
        gbps = C.c_double()
        _lib.check(_lib.lib().cos_hbm_probe(0, 1, 1 << 30, 0, 10, C.byref(gbps)))      # the streaming-copy ceiling of this machine
        per = 4 if packed.value else 5
        print(json.dumps({"profile_insert": True, "packed": int(packed.value), "postings_new_array_after_insert": nnz, "merge_bytes": nnz * 2 * per,
                          "postings_new_array_after_delete": nnz - removed, "compact_bytes": (2 * nnz - removed) * per + nnz // 4,
                          "hbm_copy_ceiling_gbps": gbps.value}))
        return
    rng = np.random.default_rng(9)
    qd, qv, qo = [], [], [0]
    for _ in range(B):                                                               # bench_sparse.py's queries
        m = int(rng.integers(16, 33))
        d = np.sort(rng.choice(VOCAB, m, replace=False, p=pz_h)).astype(np.uint32)
        qd.append(d); qv.append(np.exp(0.6 * rng.standard_normal(m)).astype(np.float32)); qo.append(qo[-1] + m)
    q = (np.concatenate(qd), np.concatenate(qv), np.array(qo, np.uint32))
    out = (np.zeros((B, K), np.uint32), np.zeros((B, K), np.float32), np.zeros(B, np.uint32))
    ev = lambda: torch.cuda.Event(enable_timing=True)

    # ---- insert against destroy + create ----
    ins_wall, ins_dev, rec_wall, base_create = [], [], [], []
    h_upd = None
    for r in range(a.reps):
        t = time.perf_counter(); h = new.create(base, n0); base_create.append((time.perf_counter() - t) * 1e3)
        e0, e1 = ev(), ev()
        torch.cuda.synchronize()
        e0.record(); t = time.perf_counter()
        new.insert(h, upd)
        ins_wall.append((time.perf_counter() - t) * 1e3); e1.record(); torch.cuda.synchronize()
        ins_dev.append(e0.elapsed_time(e1))
        if r == a.reps - 1:
            h_upd = h                                                                # (c): the index that reached the merged CSR through an insert
        else:
            new.destroy(h)
        h = new.create(base, n0)
        t = time.perf_counter()
        new.destroy(h); h = new.create(merged, n)
        rec_wall.append((time.perf_counter() - t) * 1e3)
        new.destroy(h)

    # ---- search: (a) parent build, (b) this build never updated, (c) grown by insert ----
    def timed(lib, h):
        lib.search(h, q, out)
        return float(np.median([lib.search(h, q, out) for _ in range(a.search_reps)]))

    def answer(lib, h):
        lib.search(h, q, out)
        c = out[2].copy(); live = np.arange(K)[None, :] < c[:, None]
        return c, out[0][live].copy(), out[1][live].view(np.uint32).copy()

    same = lambda x, y: bool(all(np.array_equal(p, r) for p, r in zip(x, y)))
    h_b = new.create(merged, n)
    par = Raw(a.parent_lib) if a.parent_lib else None
    h_a = par.create(merged, n) if par else None
    ms = {"a": [], "b": [], "c": [], "d": [], "e": []}
    for _ in range(a.rounds):
        if par:
            ms["a"].append(timed(par, h_a))
        ms["b"].append(timed(new, h_b))
        ms["c"].append(timed(new, h_upd))
    ans_b = answer(new, h_b)
    c_equals_b = same(ans_b, answer(new, h_upd))
    a_equals_b = same(ans_b, answer(par, h_a)) if par else None
    if par:
        par.destroy(h_a)
    new.destroy(h_b)

    # ---- delete: 1 000 vectors per call against destroy + create of what survives, then 10 % of the vectors for (d) ----
    del_ms, del_rec_ms, removed_per_call = [], [], []
    for r in range(a.reps):
        ids, u = dele(r * 1000, (r + 1) * 1000)
        t = time.perf_counter(); removed_per_call.append(new.delete(h_upd, ids, u)); del_ms.append((time.perf_counter() - t) * 1e3)
        surv = new.download(h_upd)
        h = new.create(merged, n)
        t = time.perf_counter()
        new.destroy(h); h = new.create(surv, n)
        del_rec_ms.append((time.perf_counter() - t) * 1e3)
        new.destroy(h)
    ids, u = dele(a.reps * 1000, n // 10)
    t = time.perf_counter(); new.delete(h_upd, ids, u); del_big_ms = (time.perf_counter() - t) * 1e3
    surv = new.download(h_upd)
    h_e = new.create(surv, n)
    for _ in range(a.rounds):
        ms["d"].append(timed(new, h_upd))
        ms["e"].append(timed(new, h_e))
    d_equals_e = same(answer(new, h_upd), answer(new, h_e))
    new.destroy(h_e)
    new.destroy(h_upd)
    res = {"bench": "sparse_update", "vectors": n, "vectors_before_insert": n0, "dimensions": int(merged[0].size), "postings": nnz, "postings_inserted": nnz_upd,
           "insert_ms_host_clock": spread(ins_wall), "insert_ms_device_events": spread(ins_dev),
           "destroy_plus_create_ms_host_clock": spread(rec_wall), "create_before_insert_ms_host_clock": spread(base_create),
           "insert_speedup_over_destroy_plus_create": spread(rec_wall)["median"] / spread(ins_wall)["median"],
           "delete_1000_vectors_ms_host_clock": spread(del_ms), "delete_destroy_plus_create_ms_host_clock": spread(del_rec_ms),
           "delete_speedup_over_destroy_plus_create": spread(del_rec_ms)["median"] / spread(del_ms)["median"],
           "postings_removed_per_delete_call": removed_per_call, "delete_10_percent_ms": del_big_ms, "postings_after_deletes": int(surv[2].size),
           "search_kernel_ms_per_256_query_batch": {key: spread(v) for key, v in ms.items() if v}, "search_reps_per_round": a.search_reps,
           "search_c_equals_b_bits": c_equals_b, "search_parent_equals_b_bits": a_equals_b, "search_d_equals_fresh_create_bits": d_equals_e}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
