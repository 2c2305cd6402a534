"""ID-range sharding across the GPUs of one node.

One process per GPU; shard s owns the contiguous internal ids [s*n, (s+1)*n) with its own graph
(cos_params.id_base = s*n), every query goes to every shard, each shard runs walk + local exact rerank
and emits its local top-k as (global id, cosine score).  The ONLY exchange step on the path is one
all-gather of those lists (RCCL over xGMI when the backend is "nccl"; "gloo" in the CPU tests) followed
by the S-way merge kernel (cos_merge_topk_device).  The reference has no sharding; parity for S > 1 is
defined against the oracle running the same S-shard scheme.
"""
from __future__ import annotations

import torch
import torch.distributed as dist


def shard_range(n_total: int, world: int, rank: int):
    """Contiguous id range of shard `rank` (ids are allocated sequentially, collection.rs:451-468)."""
    base = n_total // world
    lo = rank * base
    hi = n_total if rank == world - 1 else lo + base
    return lo, hi


def slice_row_masks(bits, bounds):
    """A packed mask over the GLOBAL rows of a sharded collection -> one packed mask per shard over the shard's OWN rows (what
    cos_shardset_flat_search_batch / cos_shardset_bruteforce_topk take).  Pure numpy.
    bits    uint32 [n_masks][>= ceil(N / 32)] (or one row), the layout of cos_scan_mask::bits: bit r % 32 of word r / 32 = global row r
    bounds  [S + 1] ascending row numbers; shard s holds the global rows [bounds[s], bounds[s + 1]) and N = bounds[S]
    -> list of S uint32 arrays [n_masks][ceil(n_s / 32)]: bit j of shard s = global bit bounds[s] + j; padding bits are 0, bits of the
    input at or past N are ignored.  Shard boundaries are generally not multiples of 32, so a shard's words straddle the global ones."""
    import numpy as np
    b = np.atleast_2d(np.asarray(bits))
    if b.dtype != np.uint32 or b.ndim != 2:
        raise ValueError("bits must be uint32 [n_masks][words]")
    bounds = [int(x) for x in bounds]
    if len(bounds) < 2 or bounds[0] < 0 or any(hi < lo for lo, hi in zip(bounds, bounds[1:])):
        raise ValueError("bounds must be ascending row numbers, at least two of them")
    if b.shape[1] * 32 < bounds[-1]:
        raise ValueError(f"the mask holds {b.shape[1] * 32} bits, the bounds end at row {bounds[-1]}")
    G = b.shape[0]
    src = np.zeros((G, b.shape[1] + 2), np.uint64)          # two zero words behind the end: the reads below never leave it
    src[:, :b.shape[1]] = b
    out = []
    for lo, hi in zip(bounds, bounds[1:]):
        n = hi - lo
        words = (n + 31) // 32
        w0, sh = lo // 32, lo % 32
        lo_part = src[:, w0:w0 + words] >> np.uint64(sh)    # shard word j = global bits [lo + 32 j, lo + 32 j + 32)
        hi_part = (src[:, w0 + 1:w0 + words + 1] << np.uint64(32 - sh)) & np.uint64(0xFFFFFFFF)   # (sh = 0: shifted out entirely)
        m = ((lo_part | hi_part) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        if n % 32:                                          # the bits past the shard's last row belong to the next shard (or to nobody)
            m[:, -1] &= np.uint32((1 << (n % 32)) - 1)
        out.append(np.ascontiguousarray(m))
    return out


def allgather_topk(ids: torch.Tensor, scores: torch.Tensor, counts: torch.Tensor, out_ids=None, out_scores=None, out_counts=None):
    """ids/scores [B][k], counts [B] of this shard -> gathered [S][B][k], [S][B][k], [S][B] on every rank.
    Payload per rank: B*k*8 + B*4 bytes (20 KB at B=256, k=10): latency-bound, far below xGMI bandwidth."""
    world = dist.get_world_size()
    B, k = ids.shape
    if out_ids is None:
        out_ids = torch.empty(world, B, k, dtype=ids.dtype, device=ids.device)
        out_scores = torch.empty(world, B, k, dtype=scores.dtype, device=scores.device)
        out_counts = torch.empty(world, B, dtype=counts.dtype, device=counts.device)
    # outputs viewed as the concatenation along dim 0 (the layout both the nccl and the gloo backend accept)
    dist.all_gather_into_tensor(out_ids.view(world * B, k), ids.contiguous())
    dist.all_gather_into_tensor(out_scores.view(world * B, k), scores.contiguous())
    dist.all_gather_into_tensor(out_counts.view(world * B), counts.contiguous())
    return out_ids, out_scores, out_counts


def merge_topk_device(g_ids, g_scores, g_counts, out_ids, out_scores, out_counts, device_index: int, stream: int = 0):
    """S-way merge on the GPU: total_cmp score desc, larger id first on ties (same rule as everywhere else)."""
    from . import _lib
    S, B, k = g_ids.shape
    _lib.check(_lib.lib().cos_merge_topk_device(g_ids.data_ptr(), g_scores.data_ptr(), g_counts.data_ptr(), S, B, k,
                                                out_ids.data_ptr(), out_scores.data_ptr(), out_counts.data_ptr(), device_index, stream))


# ---- packed exchange: one collective per batch -----------------------------------------------------------------
def packed_words(B: int, k: int) -> int:
    """4-byte words of one shard's packed result record [ids B*k | scores B*k | counts B]."""
    return B * (2 * k + 1)


def packed_views(buf: torch.Tensor, B: int, k: int):
    """Views (ids u32-as-int32 [B][k], scores f32 [B][k], counts int32 [B]) into one packed int32 record, so the
    search kernels write straight into the buffer that is exchanged."""
    assert buf.dtype == torch.int32 and buf.numel() == packed_words(B, k) and buf.is_contiguous()
    ids = buf[: B * k].view(B, k)
    scores = buf[B * k: 2 * B * k].view(torch.float32).view(B, k)
    counts = buf[2 * B * k:]
    return ids, scores, counts


def allgather_packed(buf: torch.Tensor, out: torch.Tensor | None = None):
    """ONE all-gather of the packed record: [words] -> [S][words].  Three small collectives per batch are
    latency-bound (tens of microseconds each on xGMI); one keeps the exchange step off the critical path."""
    world = dist.get_world_size()
    if out is None:
        out = torch.empty(world * buf.numel(), dtype=buf.dtype, device=buf.device)
    dist.all_gather_into_tensor(out.view(-1), buf)
    return out.view(world, buf.numel())


def merge_topk_packed_device(g_packed, B: int, k: int, out_ids, out_scores, out_counts, device_index: int, stream: int = 0):
    from . import _lib
    S = g_packed.shape[0]
    _lib.check(_lib.lib().cos_merge_topk_packed_device(g_packed.data_ptr(), S, B, k, out_ids.data_ptr(), out_scores.data_ptr(),
                                                       out_counts.data_ptr(), device_index, stream))


def merge_lists_device(g_ids, g_scores, g_counts, out_ids, out_scores, out_counts, device_index: int, stream: int = 0):
    """merge_topk_device for up to 8192 keys per query (cos_merge_lists_device): S * k <= 1024 launches the same kernel, above it one
    workgroup per query sorts the keys in LDS; the rule and the contract are the same."""
    from . import _lib
    S, B, k = g_ids.shape
    _lib.check(_lib.lib().cos_merge_lists_device(g_ids.data_ptr(), g_scores.data_ptr(), g_counts.data_ptr(), S, B, k,
                                                 out_ids.data_ptr(), out_scores.data_ptr(), out_counts.data_ptr(), device_index, stream))


def merge_lists_packed_device(g_packed, B: int, k: int, out_ids, out_scores, out_counts, device_index: int, stream: int = 0):
    from . import _lib
    S = g_packed.shape[0]
    _lib.check(_lib.lib().cos_merge_lists_packed_device(g_packed.data_ptr(), S, B, k, out_ids.data_ptr(), out_scores.data_ptr(),
                                                        out_counts.data_ptr(), device_index, stream))


def global_topk_by_score(ids_global: torch.Tensor, scores: torch.Tensor, k: int) -> torch.Tensor:
    """Recall bookkeeping for S shards (not on the query path): every rank contributes its [Q][k'] candidate ids (global)
    with their exact scores; returns the [Q][k] ids of the best scores over all shards, identical on every rank."""
    world = dist.get_world_size()
    all_ids = [torch.zeros_like(ids_global) for _ in range(world)]
    all_s = [torch.zeros_like(scores) for _ in range(world)]
    dist.all_gather(all_ids, ids_global.contiguous())
    dist.all_gather(all_s, scores.contiguous())
    ci, cs = torch.cat(all_ids, 1), torch.cat(all_s, 1)
    return torch.gather(ci, 1, cs.topk(k, dim=1).indices)
