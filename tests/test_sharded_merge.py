"""N>1 path on CPU: world_size-2 gloo processes, each owning an ID-range shard (oracle search stands in for the
per-shard GPU search), the all-gather exchange of cosdata_amd/sharding.py, and the merge rule.  The merged result
must equal the exact top-k over the union of the shards' candidates, and — because every shard reranks with exact
f32 cosine — must be reproducible by a single process running both shards."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _total_key(x):
    """f32::total_cmp as an integer key: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN"""
    b = int(np.float32(x).view(np.int32))
    return b ^ (0x7FFFFFFF if b < 0 else 0)


def _merge_numpy(g_ids, g_sc, g_cnt, k):
    """checker for the merge rule: total_cmp desc (so +0.0 ranks before -0.0), larger id first."""
    S, B, _ = g_ids.shape
    out_ids = np.full((B, k), 0xFFFFFFFF, np.uint32)
    out_sc = np.zeros((B, k), np.float32)
    out_cnt = np.zeros(B, np.uint32)
    for b in range(B):
        ent = [(g_sc[s, b, j], int(g_ids[s, b, j])) for s in range(S) for j in range(int(g_cnt[s, b]))]
        ent.sort(key=lambda t: (_total_key(t[0]), t[1]), reverse=True)
        ent = ent[:k]
        out_cnt[b] = len(ent)
        for j, (sc, i) in enumerate(ent):
            out_ids[b, j], out_sc[b, j] = i, sc
    return out_ids, out_sc, out_cnt


def _shard_search(X, Q, lo, hi, k):
    from oracle import oracle as O
    p = O.HNSWParams(dim=X.shape[1], num_layers=4, ef_construction=48, ef_search=48, seed=11 + lo)
    ix = O.OracleIndex(p).set_vectors(np.ascontiguousarray(X[lo:hi])).build()
    ids, sc, cnt = ix.search_batch(Q, k)[:3]
    gids = np.where(np.arange(k)[None, :] < cnt[:, None], ids + lo, 0xFFFFFFFF).astype(np.uint32)  # id_base = lo
    return gids, sc, cnt


def _worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cosdata_amd.sharding import allgather_packed, allgather_topk, packed_views, packed_words, shard_range
    rng = np.random.default_rng(123)
    X = rng.uniform(-1, 1, (1200, 40)).astype(np.float32)
    Q = (X[rng.integers(0, 1200, 16)] + 0.02 * rng.standard_normal((16, 40))).astype(np.float32)
    k = 6
    lo, hi = shard_range(1200, world, rank)
    gids, sc, cnt = _shard_search(X, Q, lo, hi, k)
    g_ids, g_sc, g_cnt = allgather_topk(torch.from_numpy(gids.view(np.int32)), torch.from_numpy(sc), torch.from_numpy(cnt.view(np.int32)))
    assert g_ids.shape == (world, 16, k)
    # packed exchange (what bench.py uses): ONE collective must carry exactly the same data
    rec = torch.zeros(packed_words(16, k), dtype=torch.int32)
    p_ids, p_sc, p_cnt = packed_views(rec, 16, k)
    p_ids.copy_(torch.from_numpy(gids.view(np.int32))); p_sc.copy_(torch.from_numpy(sc)); p_cnt.copy_(torch.from_numpy(cnt.view(np.int32)))
    g_rec = allgather_packed(rec)
    assert g_rec.shape == (world, packed_words(16, k))
    for s_ in range(world):
        u_ids, u_sc, u_cnt = packed_views(g_rec[s_].contiguous(), 16, k)
        assert torch.equal(u_ids, g_ids[s_]) and torch.equal(u_sc.view(torch.int32), g_sc[s_].view(torch.int32)) and torch.equal(u_cnt, g_cnt[s_])
    np.save(os.path.join(tmp, f"gathered_{rank}.npy"), g_ids.numpy())
    m_ids, m_sc, m_cnt = _merge_numpy(g_ids.numpy().view(np.uint32), g_sc.numpy(), g_cnt.numpy().view(np.uint32), k)
    np.savez(os.path.join(tmp, f"merged_{rank}.npz"), ids=m_ids, sc=m_sc, cnt=m_cnt)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 8])
def test_allgather_merge_gloo(tmp_path, world):
    """world 2, and world 8 = the shape of BASELINE configs[3]: eight ranks, each an id-range shard, ONE packed all-gather, the
    merge rule on every rank — against the single-process restatement of the same scheme"""
    port = _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    a, b = np.load(tmp_path / "merged_0.npz"), np.load(tmp_path / "merged_1.npz")
    assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["sc"], b["sc"])   # every rank ends with the same answer
    assert np.array_equal(np.load(tmp_path / "gathered_0.npy"), np.load(tmp_path / "gathered_1.npy"))
    for r in range(2, world):
        c = np.load(tmp_path / f"merged_{r}.npz")
        assert np.array_equal(a["ids"], c["ids"]) and np.array_equal(a["sc"], c["sc"])
    # single-process restatement of the same scheme
    sys.path.insert(0, ROOT)
    from cosdata_amd.sharding import shard_range
    rng = np.random.default_rng(123)
    X = rng.uniform(-1, 1, (1200, 40)).astype(np.float32)
    Q = (X[rng.integers(0, 1200, 16)] + 0.02 * rng.standard_normal((16, 40))).astype(np.float32)
    k = 6
    parts = [_shard_search(X, Q, *shard_range(1200, world, r), k) for r in range(world)]
    g_ids = np.stack([p[0] for p in parts]); g_sc = np.stack([p[1] for p in parts]); g_cnt = np.stack([p[2] for p in parts])
    m_ids, m_sc, m_cnt = _merge_numpy(g_ids, g_sc, g_cnt, k)
    assert np.array_equal(m_ids, a["ids"]) and np.array_equal(m_sc.view(np.uint32), a["sc"].view(np.uint32))
    # ids are global and each comes from the shard that owns it
    lo1, _ = shard_range(1200, world, 1)
    assert ((a["ids"] < 1200) | (a["ids"] == 0xFFFFFFFF)).all() and (a["ids"] >= lo1).any() and (a["ids"] < lo1).any()
    owners = {int(np.searchsorted([shard_range(1200, world, r)[1] for r in range(world)], i, side="right")) for i in a["ids"].ravel() if i != 0xFFFFFFFF}
    assert owners == set(range(world))                   # every shard contributes to somebody's merged list
    # quality: merged result vs exact brute force over the whole corpus
    from oracle import oracle as O
    gt, _ = O.bruteforce_topk(X, Q, k)
    recall = np.mean([len(set(a["ids"][i]) & set(gt[i])) / k for i in range(16)])
    assert recall >= 0.85


def test_shard_range_partition():
    from cosdata_amd.sharding import shard_range
    for n, w in [(100, 8), (12_500_000 * 8, 8), (7, 2)]:
        r = [shard_range(n, w, i) for i in range(w)]
        assert r[0][0] == 0 and r[-1][1] == n and all(r[i][1] == r[i + 1][0] for i in range(w - 1))


def test_merge_checker_orders_by_total_cmp():
    """the checker itself: -0.0 sorts below +0.0 whatever the ids, negatives below both, equal bits by the larger id"""
    sc = np.array([[[0.5, 0.0, -0.0, -0.25]], [[0.0, -0.0, -0.0, -0.5]]], np.float32)
    ids = np.array([[[1, 2, 90, 4]], [[5, 6, 7, 8]]], np.uint32)
    m_ids, m_sc, m_cnt = _merge_numpy(ids, sc, np.full((2, 1), 4, np.uint32), 8)
    assert m_ids[0].tolist() == [1, 5, 2, 90, 7, 6, 4, 8] and m_cnt[0] == 8
    assert m_sc[0].view(np.uint32).tolist() == np.array([0.5, 0.0, 0.0, -0.0, -0.0, -0.0, -0.25, -0.5], np.float32).view(np.uint32).tolist()


# S, B, k, counts ("random" | "zero" | "full"), scores ("ties": a few positive values | "signed": negatives, -0.0 and +0.0 among them).
# S*k picks the instantiation of merge_topk_kernel<R>: <= 64 R=1, <= 128 R=2, <= 256 R=4, <= 512 R=8, <= 1024 R=16.
MERGE_CASES = [(2, 33, 10, "random", "ties"), (8, 256, 10, "random", "ties"), (4, 7, 50, "random", "ties"), (8, 5, 100, "random", "ties"),
               (8, 9, 40, "random", "ties"),          # 320: R = 8
               (8, 9, 40, "full", "signed"),          # 320 live entries
               (8, 5, 8, "full", "signed"),           # 64: last size of R = 1
               (2, 3, 64, "full", "ties"),            # 128: last size of R = 2
               (8, 4, 128, "full", "signed"),         # 1024: last size of R = 16
               (4, 3, 64, "random", "signed"),        # 256: last size of R = 4
               (8, 3, 64, "full", "signed"),          # 512: last size of R = 8
               (1, 6, 10, "random", "signed"), (1, 2, 300, "full", "ties"),   # S = 1
               (8, 11, 1, "random", "signed"), (1, 4, 1, "full", "ties"),     # k = 1
               (4, 5, 20, "zero", "ties"),            # every count 0
               (3, 70, 33, "random", "signed")]
PAT_I, PAT_S = 0x5A5A5A5A, -123.25                    # what the outputs hold before the call


def _merge_inputs(rng, S, B, k, counts, scores):
    if scores == "ties":
        pool = np.linspace(0.1, 0.9, 23).astype(np.float32)
    else:
        pool = np.concatenate([np.linspace(-0.9, 0.9, 19), [0.0, -0.0, 0.0, -0.0, -1e-30, 1e-30]]).astype(np.float32)
    sc = rng.choice(pool, (S, B, k))
    keys = np.vectorize(_total_key)(sc)                               # a shard emits its list in total_cmp order: +0.0 ahead of -0.0
    sc = np.take_along_axis(sc, np.argsort(-keys, axis=2, kind="stable"), axis=2)
    ids = rng.permutation(S * B * k).astype(np.uint32).reshape(S, B, k)
    cnt = {"random": rng.integers(0, k + 1, (S, B)), "zero": np.zeros((S, B)), "full": np.full((S, B), k)}[counts].astype(np.uint32)
    return ids, sc, cnt


@pytest.mark.gpu
def test_merge_kernel_matches_rule():
    import cosdata_amd  # noqa: F401
    from cosdata_amd import _lib
    from cosdata_amd.sharding import merge_topk_device, merge_topk_packed_device
    rng = np.random.default_rng(5)
    dev = torch.device("cuda:0")
    t = lambda a, dt: torch.from_numpy(a.view(dt) if a.dtype != np.float32 else a).to(dev)
    outs = lambda B, k: (torch.full((B, k), PAT_I, dtype=torch.int32, device=dev), torch.full((B, k), PAT_S, dtype=torch.float32, device=dev),
                         torch.full((B,), PAT_I, dtype=torch.int32, device=dev))
    for S, B, k, counts, scores in MERGE_CASES:
        ids, sc, cnt = _merge_inputs(rng, S, B, k, counts, scores)
        exp = _merge_numpy(ids, sc, cnt, k)
        o_i, o_s, o_c = outs(B, k)
        merge_topk_device(t(ids, np.int32), t(sc, np.float32), t(cnt, np.int32), o_i, o_s, o_c, 0, 0)
        torch.cuda.synchronize()
        # packed per-shard records [ids | scores | counts] through cos_merge_topk_packed_device
        packed = np.concatenate([ids.reshape(S, -1).view(np.int32), sc.reshape(S, -1).view(np.int32), cnt.view(np.int32)], axis=1)
        p_i, p_s, p_c = outs(B, k)
        merge_topk_packed_device(torch.from_numpy(np.ascontiguousarray(packed)).to(dev), B, k, p_i, p_s, p_c, 0, 0)
        torch.cuda.synchronize()
        for (r_i, r_s, r_c) in [(o_i, o_s, o_c), (p_i, p_s, p_c)]:
            gc = r_c.cpu().numpy().view(np.uint32)
            gi, gs = r_i.cpu().numpy().view(np.uint32), r_s.cpu().numpy()
            assert np.array_equal(gc, exp[2]), (S, B, k)
            assert np.array_equal(gc, np.minimum(cnt.sum(axis=0), k))
            for b in range(B):
                c = int(gc[b])
                assert np.array_equal(gi[b, :c], exp[0][b, :c]), (S, B, k, b)
                assert np.array_equal(gs[b, :c].view(np.uint32), exp[1][b, :c].view(np.uint32)), (S, B, k, b)   # bits: -0.0 is not +0.0
                assert (gi[b, c:] == PAT_I).all() and (gs[b, c:] == np.float32(PAT_S)).all(), (S, B, k, b, "slots past count were written")
    # S*k = 1025: one past the widest instantiation — refused, nothing written
    for S, B, k in [(5, 3, 205), (1, 2, 1025)]:
        ids, sc, cnt = _merge_inputs(rng, S, B, k, "full", "ties")
        packed = np.concatenate([ids.reshape(S, -1).view(np.int32), sc.reshape(S, -1).view(np.int32), cnt.view(np.int32)], axis=1)
        o_i, o_s, o_c = outs(B, k)
        with pytest.raises(_lib.CosdataError) as ei:
            merge_topk_device(t(ids, np.int32), t(sc, np.float32), t(cnt, np.int32), o_i, o_s, o_c, 0, 0)
        assert ei.value.status == 4                      # COS_ERR_UNIMPLEMENTED
        with pytest.raises(_lib.CosdataError) as ei:
            merge_topk_packed_device(torch.from_numpy(np.ascontiguousarray(packed)).to(dev), B, k, o_i, o_s, o_c, 0, 0)
        assert ei.value.status == 4
        torch.cuda.synchronize()
        assert (o_i == PAT_I).all() and (o_s == PAT_S).all() and (o_c == PAT_I).all()


def _recall_worker(rank, world, port, tmp):
    """bench.py's recall bookkeeping for N > 1, on CPU: per-shard exact top-k (global ids) -> global_topk_by_score ->
    every rank holds the same global ground truth, equal to the single-process brute force over the whole corpus."""
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cosdata_amd.sharding import global_topk_by_score, shard_range
    from oracle import oracle as O
    rng = np.random.default_rng(77)
    n, d, nq, k = 900, 24, 10, 5
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    lo, hi = shard_range(n, world, rank)
    lid, _ = O.bruteforce_topk(np.ascontiguousarray(X[lo:hi]), Q, k)
    gids = torch.from_numpy(lid.astype(np.int64) + lo)
    Xt, Qt = torch.from_numpy(X), torch.from_numpy(Q)
    sims = torch.einsum("qd,qkd->qk", Qt, Xt[gids])           # what bench.py::merge_global computes
    merged = global_topk_by_score(gids, sims, k)
    np.save(os.path.join(tmp, f"gt_{rank}.npy"), merged.numpy())
    r = torch.tensor([0.5 + rank])                            # the ef decision is broadcast from rank 0
    dist.broadcast(r, 0)
    assert float(r.item()) == 0.5
    t = torch.tensor([1.0 + rank], dtype=torch.float64)       # timed region: MAX over ranks
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    assert float(t.item()) == float(world)
    dist.barrier()
    dist.destroy_process_group()


def test_global_ground_truth_merge_gloo(tmp_path):
    world = 2
    mp.spawn(_recall_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    a, b = np.load(tmp_path / "gt_0.npy"), np.load(tmp_path / "gt_1.npy")
    assert np.array_equal(a, b)
    from oracle import oracle as O
    rng = np.random.default_rng(77)
    X = rng.standard_normal((900, 24)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = rng.standard_normal((10, 24)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    gt, _ = O.bruteforce_topk(X, Q, 5)
    assert all(set(a[i].tolist()) == set(gt[i].tolist()) for i in range(10))
