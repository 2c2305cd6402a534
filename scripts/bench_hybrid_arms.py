#!/usr/bin/env python3
"""The mixed hybrid call (cos_hybrid_search_mixed) against the composition a host without it runs: separate host-buffer searches of
the halves an arm names, each for top_k * 3, then cos_rrf_fuse_batch.  Corpus: config c5's dense and BM25 side (scripts/bench_c5.py)
plus a learned-sparse index over the same ids, generated like scripts/bench_sparse.py (Zipf dimensions, log-normal values, 6-bit keys,
raw vectors kept for the rerank).  256-query batches; the three uniform arms and an even mix (arms cycling 0, 1, 2); every shape is
warmed up, then the two sides alternate in the same process for `--rounds` rounds of `--reps` batches; ms per batch is the median
of the rounds, spread = max - min.  Also: the all-DENSE_BM25 mixed call against cos_hybrid_search_batch.  One JSON line."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def build(n, dim, vocab, doc_len, sparse_vocab, sparse_nnz, device=0):
    import torch
    import cosdata_amd as ca
    import bench
    dev = torch.device(f"cuda:{device}")
    g = torch.Generator(device=dev); g.manual_seed(11)
    # ---- dense side (scripts/bench_c5.py) ----
    nc = max(64, n // 1000)
    centers = torch.randn(nc, dim, generator=g, device=dev); centers /= centers.norm(dim=1, keepdim=True)
    X = bench.mixture(torch, n, dim, 42, dev, centers)
    ix = ca.HNSWIndex(dim, ca.HNSWHyperParams(), ca.DistanceMetric.Cosine, ca.StorageType.UnsignedByte(), (-1.0, 1.0), device=device)
    ix.upload_vectors_device(X.data_ptr(), n, keepalive=X)
    ix.build(4096)
    # ---- text side (scripts/bench_c5.py): Zipf tokens -> CSR postings with stored BM25 tf ----
    V = vocab
    pz = 1.0 / torch.arange(1, V + 1, device=dev, dtype=torch.float64) ** 1.1; pz /= pz.sum()
    lens = torch.poisson(torch.full((n,), doc_len, device=dev), generator=g).clamp_(min=1).to(torch.int64)
    doc_of_tok = torch.repeat_interleave(torch.arange(n, device=dev), lens)
    term_rank = torch.searchsorted(torch.cumsum(pz, 0), torch.rand(int(lens.sum().item()), generator=g, device=dev, dtype=torch.float64)).clamp_(max=V - 1)
    hashes = torch.unique(torch.randint(0, 1 << 31, (V * 2,), generator=g, device=dev, dtype=torch.int64))[:V]
    ukey, counts = torch.unique(term_rank * n + doc_of_tok, return_counts=True)
    p_term = ukey // n; p_doc = (ukey % n).to(torch.int32)
    c = counts.to(torch.float32); dl = lens[p_doc.long()].to(torch.float32)
    tf = c * 2.5 / (c + 1.5 * (0.25 + 0.75 * (dl / float(lens.double().mean().item()))))
    offsets = torch.zeros(V + 1, dtype=torch.int64, device=dev); offsets[1:] = torch.cumsum(torch.bincount(p_term, minlength=V), 0)
    th_h = hashes.cpu().numpy().astype(np.uint32)
    bm = ca.BM25Index(th_h, offsets.cpu().numpy().astype(np.uint64), p_doc.cpu().numpy().astype(np.uint32), tf.cpu().numpy().astype(np.float32), n, device=device)
    del ukey, counts, term_rank, doc_of_tok, p_term, c, dl
    # ---- learned-sparse side (scripts/bench_sparse.py) as raw vectors: the library files them by (dimension, quantized value) ----
    ps = 1.0 / torch.arange(1, sparse_vocab + 1, device=dev, dtype=torch.float64) ** 0.9
    sdim = torch.searchsorted(torch.cumsum(ps / ps.sum(), 0), torch.rand(n * sparse_nnz, generator=g, device=dev, dtype=torch.float64)).clamp_(max=sparse_vocab - 1)
    vid = torch.arange(n, device=dev).repeat_interleave(sparse_nnz)
    pair = torch.unique(vid * sparse_vocab + sdim)                        # one pair per (vector, dimension), dimensions ascending inside a vector
    vid, sdim = pair // sparse_vocab, pair % sparse_vocab
    val = torch.exp(0.6 * torch.randn(pair.numel(), generator=g, device=dev)).clamp_(max=3.0 * 1.2).float()
    row_off = torch.zeros(n + 1, dtype=torch.int64, device=dev); row_off[1:] = torch.cumsum(torch.bincount(vid, minlength=n), 0)
    sp = ca.InvertedIndex.from_vectors(6, 3.0, row_off.cpu().numpy().astype(np.uint64), sdim.cpu().numpy().astype(np.uint32), val.cpu().numpy(), keep_raw=True,
                                       device=device)
    Q = bench.mixture(torch, 256, dim, 43, dev, centers).cpu().numpy()
    return ix, bm, sp, Q, th_h, pz.cpu().numpy(), (ps / ps.sum()).cpu().numpy(), int(offsets[-1].item()), int(pair.numel())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--sparse-vocab", type=int, default=30_000)
    ap.add_argument("--sparse-nnz", type=int, default=48)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--rerank", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", help="append the JSON line to this file too")
    a = ap.parse_args()
    import cosdata_amd as ca
    t_all = time.time()
    B, k, rf, k3 = a.batch, a.top_k, a.rerank, 3 * a.top_k
    ix, bm, sp, Q, th_h, pz_h, ps_h, bm_postings, sp_postings = build(a.n, a.dim, a.vocab, 120.0, a.sparse_vocab, a.sparse_nnz)
    sp.set_max_candidates(min(1024, k3 * max(rf, 1)))
    ctx = ca.HybridContext()
    rng = np.random.default_rng(5)
    bq = [th_h[rng.choice(a.vocab, int(rng.integers(2, 9)), replace=False, p=pz_h)].astype(np.uint32) for _ in range(B)]
    sq = []
    for _ in range(B):
        m = int(rng.integers(16, 33))
        sq.append((np.sort(rng.choice(a.sparse_vocab, m, replace=False, p=ps_h)).astype(np.uint32), np.exp(0.6 * rng.standard_normal(m)).astype(np.float32)))

    def shape(arms):
        """the request of a batch whose query q takes arm arms[q], and the index arrays the composition gathers its lists with"""
        arms = np.asarray(arms, np.uint8)
        has_d, has_s, has_b = arms != 2, arms != 1, arms != 0
        dense = Q[has_d] if has_d.any() else None
        s_sel = [sq[q] for q in range(B) if has_s[q]]
        sparse = (np.concatenate([d for d, _ in s_sel]), np.concatenate([v for _, v in s_sel]), np.cumsum([0] + [d.size for d, _ in s_sel]).astype(np.uint32)) if s_sel else None
        b_sel = [bq[q] for q in range(B) if has_b[q]]
        bm25 = (np.concatenate(b_sel), np.cumsum([0] + [t.size for t in b_sel]).astype(np.uint32)) if b_sel else None
        pos = {"d": np.cumsum(has_d) - 1, "s": np.cumsum(has_s) - 1, "b": np.cumsum(has_b) - 1}      # the running counts of query_mapping
        return arms, dense, sparse, bm25, pos

    def one_call(s):
        arms, dense, sparse, bm25, _ = s
        return ca.hybrid_search_mixed(ctx, ix if dense is not None else None, sp if sparse is not None else None, bm if bm25 is not None else None,
                                      arms, dense, sparse, bm25, k, 60.0, 0.0, rf)

    def composition(s):
        arms, dense, sparse, bm25, pos = s
        first = np.zeros((B, k3), np.uint32); second = np.zeros((B, k3), np.uint32)
        fc = np.zeros(B, np.uint32); sc = np.zeros(B, np.uint32)
        if dense is not None:
            di, _, dc = ix.batch_search(dense, k3)[:3]
            m = arms != 2
            first[m], fc[m] = di, dc
        if sparse is not None:
            si, _, scn = sp.search_batch(*sparse, k3, 0.0, rf)
            m = arms == 0
            second[m], sc[m] = si[pos["s"][m]], scn[pos["s"][m]]
            m = arms == 2
            first[m], fc[m] = si[pos["s"][m]], scn[pos["s"][m]]
        if bm25 is not None:
            bi, _, bc = bm.search_batch(*bm25, k3)
            m = arms != 0
            second[m], sc[m] = bi[pos["b"][m]], bc[pos["b"][m]]
        return ca.rrf_fuse_batch(first, fc, second, sc, 60.0, k)

    def same(x, y):
        live = np.arange(k)[None, :] < y[2][:, None]
        return bool(np.array_equal(x[2], y[2]) and np.array_equal(x[0][live], y[0][live]) and np.array_equal(x[1][live].view(np.uint32), y[1][live].view(np.uint32)))

    def timed(fn):
        t = time.perf_counter()
        for _ in range(a.reps):
            fn()
        return (time.perf_counter() - t) / a.reps * 1e3

    def versus(f_a, f_b):
        for _ in range(2):                                                 # warm up both sides of the shape
            ra, rb = f_a(), f_b()
        ta, tb = [], []
        for _ in range(a.rounds):
            ta.append(timed(f_a)); tb.append(timed(f_b))
        stat = lambda t: {"ms_per_batch": float(np.median(t)), "spread_ms": float(max(t) - min(t)), "rounds_ms": [float(x) for x in t]}
        return stat(ta), stat(tb), same(ra, rb)

    shapes = {"dense_sparse": [0] * B, "dense_bm25": [1] * B, "sparse_bm25": [2] * B, "even_mix": [q % 3 for q in range(B)]}
    out = {"config": {"workload": f"mixed hybrid call vs separate searches + cos_rrf_fuse_batch: {a.n} ids, dense({a.dim}) HNSW u8, BM25 {bm_postings} postings, "
                                  f"learned-sparse {sp_postings} postings (6-bit keys), batch {B}, top_k {k}, reranking_factor {rf}",
                      "docs": a.n, "dim": a.dim, "query_batch": B, "top_k": k, "reranking_factor": rf, "rounds": a.rounds, "reps_per_round": a.reps},
           "shapes": {}}
    for name, arms in shapes.items():
        s = shape(arms)
        one, comp, equal = versus(lambda: one_call(s), lambda: composition(s))
        out["shapes"][name] = {"one_call": one, "composition": comp, "one_call_equals_composition": equal,
                               "one_call_not_slower": one["ms_per_batch"] <= comp["ms_per_batch"]}
    s = shape(shapes["dense_bm25"])
    one, old, equal = versus(lambda: one_call(s), lambda: ca.hybrid_search_batch(ix, bm, s[1], s[3][0], s[3][1], k, 60.0))
    spread = max(one["spread_ms"], old["spread_ms"])
    out["dense_bm25_vs_cos_hybrid_search_batch"] = {"mixed": one, "cos_hybrid_search_batch": old, "equal": equal, "difference_ms": one["ms_per_batch"] - old["ms_per_batch"],
                                                   "within_three_spreads": abs(one["ms_per_batch"] - old["ms_per_batch"]) <= 3 * spread}
    out["seconds"] = time.time() - t_all
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
