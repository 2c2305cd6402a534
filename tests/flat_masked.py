"""The world of the masked exhaustive-scan tests (test_gpu_flat_masked.py on the device, test_flat_masked_cpu.py without one) and the
yardstick they share: the ORACLE ON THE SUBSET.  coso_flat_search_batch / coso_bruteforce_topk over X[S], with the ids mapped back
through the ascending row list S, is the scan over the live rows S bit for bit — the quantizer does not look at the corpus, and every
tie rule ("larger id first") survives a monotone id map.  Answers are cached per process: a reference is computed once and never changed."""
import numpy as np

from oracle import oracle as O
from tests import helpers as H

N, DIM, NQ, TOP_K = 20003, 128, 70, 10          # one seeded chunk (16384 rows) plus one fused chunk; two 64-dim chunks: every storage has a query-resident kernel
KEEPS = (0.5, 0.9, 0.02)
STORAGES = {"u8": (O.STORAGE_U8, 0), "binary": (O.STORAGE_SUBBYTE, 1), "quaternary": (O.STORAGE_SUBBYTE, 2), "octal": (O.STORAGE_SUBBYTE, 3)}

_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def world(dim=DIM, nq=NQ):
    """corpus [N][dim] and nq queries near it, both scaled into the quantizer's range"""
    def make():
        X = H.clustered_corpus(N, dim, n_centers=10, sigma=0.25, seed=3) * np.float32(0.9)
        Q = H.queries_from(X, nq, noise=0.05, seed=2) * np.float32(0.9)
        X.setflags(write=False)
        Q.setflags(write=False)
        return X, Q
    return _memo(("world", dim, nq), make)


def keep_mask(keep, n=N):
    m = np.random.default_rng(5).random(n) < keep
    m.setflags(write=False)
    return m


def four_masks():
    """the three keeps and all-ones: the per-query cases use query_mask[b] = b % 4"""
    return np.stack([keep_mask(k) for k in KEEPS] + [np.ones(N, bool)])


def oracle_index(X, storage, metric=O.METRIC_COSINE, values_range=(-1.0, 1.0)):
    kind, res = STORAGES[storage]
    p = O.HNSWParams(dim=X.shape[1], metric=metric, storage=kind, resolution=res, num_layers=3, range_lo=values_range[0], range_hi=values_range[1])
    return O.OracleIndex(p).set_vectors(X)


def subset_flat(X, Q, storage, live, top_k, metric=O.METRIC_COSINE, key=None, values_range=(-1.0, 1.0)):
    """the oracle's flat search over the rows X[live], ids mapped back -> (ids [B][top_k], scores, counts); counts = min(top_k, live rows),
    checked, so that a bad corpus cannot pass for a device bug.  `key` names (X, Q, live) for the cache; None = not cached.
    `values_range`: the u8 quantizer's (lo, hi); the default is the index's default."""
    def make():
        rows = np.flatnonzero(live).astype(np.uint32)
        B = Q.shape[0]
        if rows.size == 0:
            return np.full((B, top_k), 0xFFFFFFFF, np.uint32), np.zeros((B, top_k), np.float32), np.zeros(B, np.uint32)
        ids, sc, cnt = oracle_index(np.ascontiguousarray(X[rows]), storage, metric, values_range).flat_search_batch(Q, top_k, threads=8)   # raises unless COSO_OK
        assert (cnt == min(top_k, rows.size)).all()
        out = np.full_like(ids, 0xFFFFFFFF)
        for b in range(B):
            out[b, :cnt[b]] = rows[ids[b, :cnt[b]]]
        return out, sc, cnt
    return make() if key is None else _memo(("flat", key, storage, top_k, metric, tuple(values_range)), make)


def subset_brute(X, Q, live, k, key=None):
    """O.bruteforce_topk over X[live], ids mapped back -> (ids [B][k], scores, counts), counts = min(k, live rows)"""
    def make():
        rows = np.flatnonzero(live).astype(np.uint32)
        B, kk = Q.shape[0], min(k, int(np.count_nonzero(live)))
        out, sc = np.full((B, k), 0xFFFFFFFF, np.uint32), np.zeros((B, k), np.float32)
        if kk:
            ids, s = O.bruteforce_topk(np.ascontiguousarray(X[rows]), Q, kk, threads=8)
            out[:, :kk], sc[:, :kk] = rows[ids], s
        return out, sc, np.full(B, kk, np.uint32)
    return make() if key is None else _memo(("brute", key, k), make)


def same(got, ref, rows=None, what=None):
    """counts, ids and score BITS of the first counts[b] entries; `rows` = the queries of `ref` that `got` holds (default: its first len(got))"""
    ids, sc, cnt = (np.asarray(a) for a in got[:3])
    sel = np.arange(ids.shape[0]) if rows is None else np.asarray(rows)
    oids, osc, ocnt = (np.asarray(a)[sel] for a in ref[:3])
    assert np.array_equal(cnt, ocnt), (what, cnt, ocnt)
    for b in range(ids.shape[0]):
        c = int(cnt[b])
        assert np.array_equal(ids[b, :c], oids[b, :c]), (what, b, ids[b, :c], oids[b, :c])
        assert np.array_equal(np.ascontiguousarray(sc[b, :c]).view(np.uint32), np.ascontiguousarray(osc[b, :c]).view(np.uint32)), (what, b)


def mask_matters(full_ids, live):
    """queries whose UNMASKED top list holds a row outside `live`: filtering after the scan would have to drop something there"""
    return int(sum((~live[full_ids[b]]).any() for b in range(full_ids.shape[0])))
