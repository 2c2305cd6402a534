#!/usr/bin/env python3
"""Updates of the resident BM25 postings on c5's text corpus (1M documents, Zipf(1.1) vocabulary of 200k term hashes, document
length ~Poisson(120): the generator of scripts/bench_c5.py), one JSON line:

  insert   100 000 documents into the 900 000-document index (cos_bm25_insert) against the only way without it:
           cos_bm25_destroy + cos_bm25_create from the merged host CSR (the host-side merge is not even counted).  Same process,
           alternated, `--reps` repetitions each; medians and spread.
  search   cos_bm25_search_batch_device of c5's 256-query batch on (b) a never-updated index, (c) an index that reached the same
           CSR through the insert, (d) the same with 10 % of the documents tombstoned — and, with --parent-lib PATH (another
           build of libcosdata_hip.so, e.g. the parent commit's), (a) that build on the never-updated index, alternated with (b)
           round by round so that the spread of each against itself is known.
  delete   1 000 documents per call.

--profile-insert: one create + one insert and nothing else — the run to put under `rocprofv3 --kernel-trace --stats` for the
merge kernel's own time (16 B per posting of the new array over that time against the 8 TB/s HBM peak)."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_PEAK_GBPS = 8000.0


def text_corpus(torch, dev, n, V, doc_len, seed=11):
    """bench_c5's text side -> term-major CSR on the host + (doc, term rank) pairs for the document-major view"""
    g = torch.Generator(device=dev); g.manual_seed(seed)
    ranks = torch.arange(1, V + 1, device=dev, dtype=torch.float64)
    pz = (1.0 / ranks ** 1.1); pz /= pz.sum()
    lens = torch.poisson(torch.full((n,), doc_len, device=dev), generator=g).clamp_(min=1).to(torch.int64)
    tot = int(lens.sum().item())
    doc_of_tok = torch.repeat_interleave(torch.arange(n, device=dev), lens)
    cdf = torch.cumsum(pz, 0)
    term_rank = torch.searchsorted(cdf, torch.rand(tot, generator=g, device=dev, dtype=torch.float64)).clamp_(max=V - 1)
    hashes = torch.unique(torch.randint(0, 1 << 31, (V * 2,), generator=g, device=dev, dtype=torch.int64))[:V]
    assert hashes.numel() == V
    ukey, counts = torch.unique(term_rank * n + doc_of_tok, return_counts=True)     # sorted by (term, doc)
    del term_rank, doc_of_tok
    p_term = ukey // n; p_doc = ukey % n
    avg_len = float(lens.double().mean().item())
    c = counts.to(torch.float32); dl = lens[p_doc].to(torch.float32)
    tf = c * 2.5 / (c + 1.5 * (0.25 + 0.75 * (dl / avg_len)))                       # compute_bm25_term_frequency, k1 1.5, b 0.75
    return hashes, p_term, p_doc, tf, pz


def csr_of(torch, V, hashes, p_term, p_doc, tf, mask=None):
    if mask is not None:
        p_term, p_doc, tf = p_term[mask], p_doc[mask], tf[mask]
    df = torch.bincount(p_term, minlength=V)
    keep = df > 0                                                                    # terms with a posting in this slice
    off = torch.zeros(int(keep.sum().item()) + 1, dtype=torch.int64, device=p_term.device)
    off[1:] = torch.cumsum(df[keep], 0)
    return (hashes[keep].cpu().numpy().astype(np.uint32), off.cpu().numpy().astype(np.uint64), p_doc.cpu().numpy().astype(np.uint32),
            tf.cpu().numpy().astype(np.float32))


def doc_major(torch, V, hashes, p_term, p_doc, tf, lo, hi):
    """documents [lo, hi) as cos_bm25_insert takes them: ids, offsets, term hashes ascending inside a document, tfs"""
    m = (p_doc >= lo) & (p_doc < hi)
    t, d, f = p_term[m], p_doc[m], tf[m]
    o = torch.argsort(d * V + t)
    d, t, f = d[o], t[o], f[o]
    off = torch.searchsorted(d, torch.arange(lo, hi + 1, device=d.device))
    return (np.arange(lo, hi, dtype=np.uint32), off.cpu().numpy().astype(np.uint64), hashes[t].cpu().numpy().astype(np.uint32),
            f.cpu().numpy().astype(np.float32))


class Raw:
    """the BM25 entry points of ONE build of the library through plain ctypes (two builds can be loaded side by side)"""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.has_update = hasattr(self.L, "cos_bm25_insert")
        for name in ("cos_bm25_create", "cos_bm25_destroy", "cos_bm25_search_batch_device", "cos_bm25_insert", "cos_bm25_delete"):
            if hasattr(self.L, name):
                getattr(self.L, name).restype = C.c_int32
        self.L.cos_last_error_string.restype = C.c_char_p

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.L.cos_last_error_string().decode())

    @staticmethod
    def p(a):
        return a.ctypes.data_as(C.c_void_p)

    def create(self, csr, n_docs):
        h = C.c_void_p()
        self.ok(self.L.cos_bm25_create(C.c_int32(0), self.p(csr[0]), self.p(csr[1]), C.c_uint32(csr[0].size), self.p(csr[2]), self.p(csr[3]),
                                       C.c_uint32(n_docs), C.byref(h)))
        return h

    def destroy(self, h):
        self.ok(self.L.cos_bm25_destroy(h))

    def insert(self, h, u):
        self.ok(self.L.cos_bm25_insert(h, self.p(u[0]), self.p(u[1]), C.c_uint32(u[0].size), self.p(u[2]), self.p(u[3])))

    def delete(self, h, u):
        self.ok(self.L.cos_bm25_delete(h, self.p(u[0]), self.p(u[1]), C.c_uint32(u[0].size), self.p(u[2])))

    def search_device(self, h, qt, qo, k, o_i, o_s, o_c, stream):
        self.ok(self.L.cos_bm25_search_batch_device(h, self.p(qt), self.p(qo), C.c_uint32(qo.size - 1), C.c_uint32(k), C.c_void_p(o_i.data_ptr()),
                                                    C.c_void_p(o_s.data_ptr()), C.c_void_p(o_c.data_ptr()), C.c_void_p(stream)))


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--doc-len", type=float, default=120.0)
    ap.add_argument("--grow", type=float, default=0.1, help="share of the documents that arrives through cos_bm25_insert")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7, help="alternations of the search comparison")
    ap.add_argument("--search-reps", type=int, default=20, help="search calls per round")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--profile-insert", action="store_true")
    a = ap.parse_args()
    import torch
    from cosdata_amd import _lib
    dev = torch.device("cuda:0")
    n, V, B, k = a.docs, a.vocab, 256, 30
    n0 = n - int(n * a.grow)
    hashes, p_term, p_doc, tf, pz = text_corpus(torch, dev, n, V, a.doc_len)
    merged = csr_of(torch, V, hashes, p_term, p_doc, tf)
    base = csr_of(torch, V, hashes, p_term, p_doc, tf, p_doc < n0)
    upd = doc_major(torch, V, hashes, p_term, p_doc, tf, n0, n)
    th_all = hashes.cpu().numpy().astype(np.uint32)
    new = Raw(_lib.SO_PATH)
    if a.profile_insert:
        h = new.create(base, n0)
        new.insert(h, upd)
        new.destroy(h)
        gbps = C.c_double()
        _lib.check(_lib.lib().cos_hbm_probe(0, 1, 1 << 30, 0, 10, C.byref(gbps)))      # the streaming-copy ceiling of this machine
        print(json.dumps({"profile_insert": True, "postings_new_array": int(merged[2].size), "merge_bytes": int(merged[2].size) * 16,
                          "hbm_copy_ceiling_gbps": gbps.value}))
        return
    rng = np.random.default_rng(5)
    pz_h = pz.cpu().numpy()
    qt, qo = [], [0]
    for _ in range(B):                                                               # bench_c5's queries: 2-8 terms, Zipf-distributed
        m = int(rng.integers(2, 9))
        qt.append(th_all[rng.choice(V, m, replace=False, p=pz_h)]); qo.append(qo[-1] + m)
    qt, qo = np.concatenate(qt).astype(np.uint32), np.array(qo, np.uint32)
    all_docs = doc_major(torch, V, hashes, p_term, p_doc, tf, 0, n)                 # every document's term hashes, for the deletes
    del p_term, p_doc, tf
    torch.cuda.empty_cache()
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

    # ---- search: (a) parent build, (b) this build never updated, (c) grown by insert, (d) 10 % tombstoned ----
    st = torch.cuda.Stream(device=dev)
    o_i = torch.zeros(B, k, dtype=torch.int32, device=dev); o_s = torch.zeros(B, k, device=dev); o_c = torch.zeros(B, dtype=torch.int32, device=dev)

    def timed(lib, h):
        lib.search_device(h, qt, qo, k, o_i, o_s, o_c, st.cuda_stream)
        e0, e1 = ev(), ev()
        e0.record(st)
        for _ in range(a.search_reps):
            lib.search_device(h, qt, qo, k, o_i, o_s, o_c, st.cuda_stream)
        e1.record(st); st.synchronize()
        return e0.elapsed_time(e1) / a.search_reps

    def answer(lib, h):
        lib.search_device(h, qt, qo, k, o_i, o_s, o_c, st.cuda_stream); st.synchronize()
        c = o_c.cpu().numpy(); live = np.arange(k)[None, :] < c[:, None]
        return c.copy(), o_i.cpu().numpy()[live].copy(), o_s.cpu().numpy()[live].view(np.uint32).copy()

    same = lambda x, y: bool(all(np.array_equal(p, q) for p, q in zip(x, y)))
    h_b = new.create(merged, n)
    par = Raw(a.parent_lib) if a.parent_lib else None
    h_a = par.create(merged, n) if par else None
    ms = {"a": [], "b": [], "c": []}
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

    # ---- delete: 1 000 documents per call, then 10 % of the documents for (d) ----
    del_ms = []
    perm = np.random.default_rng(9).permutation(n)

    def docs_update(ids):
        ids = np.sort(ids).astype(np.uint32)
        lo, hi = all_docs[1][ids].astype(np.int64), all_docs[1][ids + 1].astype(np.int64)
        off = np.zeros(ids.size + 1, np.uint64); off[1:] = np.cumsum(hi - lo)
        idx = np.concatenate([np.arange(x, y) for x, y in zip(lo, hi)])
        return ids, off, all_docs[2][idx]

    for r in range(a.reps):
        u = docs_update(perm[r * 1000:(r + 1) * 1000])
        t = time.perf_counter(); new.delete(h_upd, u); del_ms.append((time.perf_counter() - t) * 1e3)
    u = docs_update(perm[a.reps * 1000:n // 10])
    t = time.perf_counter(); new.delete(h_upd, u); del_big_ms = (time.perf_counter() - t) * 1e3
    ms["d"] = [timed(new, h_upd) for _ in range(a.rounds)]
    new.destroy(h_upd)
    nnz = int(merged[2].size)
    out = {"bench": "bm25_update", "docs": n, "docs_before_insert": n0, "vocab": V, "postings": nnz, "postings_inserted": int(upd[2].size),
           "insert_ms_host_clock": spread(ins_wall), "insert_ms_device_events": spread(ins_dev),
           "destroy_plus_create_ms_host_clock": spread(rec_wall), "create_900k_ms_host_clock": spread(base_create),
           "insert_speedup_over_destroy_plus_create": spread(rec_wall)["median"] / spread(ins_wall)["median"],
           "merge_bytes": nnz * 16,
           "search_ms_per_256_query_batch": {key: spread(v) for key, v in ms.items() if v}, "search_reps_per_round": a.search_reps,
           "search_c_equals_b_bits": c_equals_b, "search_parent_equals_b_bits": a_equals_b,
           "delete_1000_docs_ms": spread(del_ms), "delete_10_percent_ms": del_big_ms, "deleted_docs_total": int(n // 10),
           "hbm_peak_gbps": HBM_PEAK_GBPS}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
