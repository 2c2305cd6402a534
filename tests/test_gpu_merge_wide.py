"""GPU: the S-way merge for up to 8192 keys per query (cos_merge_lists_device / cos_merge_lists_packed_device) against the checker of the
merge rule (tests/test_sharded_merge.py::_merge_numpy), bit for bit: every LDS width (2048, 4096, 8192 keys), both sides of the 1024-key
boundary, counts random / zero / full, scores with +0.0 and -0.0, unsorted lists, the slots past the count, and the refusal above 8192.
At 1024 keys and below the calls launch the kernel of cos_merge_topk_device: the same bits, compared output buffer for output buffer."""
import numpy as np
import pytest
import torch

from tests.test_sharded_merge import PAT_I, PAT_S, _merge_inputs, _merge_numpy

pytestmark = pytest.mark.gpu

# S, B, k, counts, scores, shuffled.  S * k picks the kernel: <= 1024 merge_topk_kernel<R>, then merge_lists_lds_kernel<N> of N = 2048, 4096, 8192
WIDE_CASES = [(8, 3, 129, "random", "ties", False),      # 1032 -> N 2048
              (8, 2, 256, "full", "signed", False),      # 2048: last size of N 2048
              (8, 2, 257, "random", "signed", False),    # 2056 -> N 4096
              (8, 3, 512, "full", "ties", False),        # 4096: last size of N 4096 (eight shards x brute-force k 512)
              (5, 4, 700, "random", "signed", False),    # 3500: S is no power of two
              (16, 2, 512, "full", "signed", False),     # 8192: last size of N 8192
              (16, 2, 512, "random", "ties", False),
              (1, 2, 1025, "full", "ties", False),       # S = 1, one key past the wave kernel
              (5, 3, 205, "random", "signed", False),    # 1025
              (8, 2, 128, "full", "signed", False),      # 1024: the wave kernel's last size
              (8, 2, 204, "zero", "ties", False),        # 1632 keys, every count 0
              (8, 3, 300, "random", "signed", True),     # every list in random order
              (3, 5, 64, "random", "signed", True)]      # ... and on the wave kernel
NARROW_SAME_BITS = [(8, 2, 128, "full", "signed"), (4, 7, 50, "random", "ties"), (1, 3, 1024, "random", "signed"), (8, 5, 8, "full", "signed")]


def _dev():
    return torch.device("cuda:0")


def _t(a, dt):
    return torch.from_numpy(a.view(dt) if a.dtype != np.float32 else a).to(_dev())


def _outs(B, k):
    dev = _dev()
    return (torch.full((B, k), PAT_I, dtype=torch.int32, device=dev), torch.full((B, k), PAT_S, dtype=torch.float32, device=dev),
            torch.full((B,), PAT_I, dtype=torch.int32, device=dev))


def _packed(ids, sc, cnt):
    S = ids.shape[0]
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([ids.reshape(S, -1).view(np.int32), sc.reshape(S, -1).view(np.int32), cnt.view(np.int32)],
                                                                axis=1))).to(_dev())


def _check(r_i, r_s, r_c, exp, cnt, k, what):
    gc = r_c.cpu().numpy().view(np.uint32)
    gi, gs = r_i.cpu().numpy().view(np.uint32), r_s.cpu().numpy()
    assert np.array_equal(gc, exp[2]), what
    assert np.array_equal(gc, np.minimum(cnt.sum(axis=0), k)), what
    for b in range(gi.shape[0]):
        c = int(gc[b])
        assert np.array_equal(gi[b, :c], exp[0][b, :c]), (what, b)
        assert np.array_equal(gs[b, :c].view(np.uint32), exp[1][b, :c].view(np.uint32)), (what, b)      # bits: -0.0 is not +0.0
        assert (gi[b, c:] == PAT_I).all() and (gs[b, c:] == np.float32(PAT_S)).all(), (what, b, "slots past the count were written")


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: "S%d-B%d-k%d-%s-%s%s" % (c[0], c[1], c[2], c[3], c[4], "-shuffled" if c[5] else ""))
def test_wide_merge_matches_rule(case):
    import cosdata_amd  # noqa: F401
    from cosdata_amd.sharding import merge_lists_device, merge_lists_packed_device
    S, B, k, counts, scores, shuffled = case
    rng = np.random.default_rng(S * 100003 + B * 1009 + k)
    ids, sc, cnt = _merge_inputs(rng, S, B, k, counts, scores)
    if shuffled:                                          # the lists may be in any order: the same permutation of ids and scores per list
        perm = np.argsort(rng.random((S, B, k)), axis=2)
        ids, sc = np.take_along_axis(ids, perm, axis=2), np.take_along_axis(sc, perm, axis=2)
    exp = _merge_numpy(ids, sc, cnt, k)
    o_i, o_s, o_c = _outs(B, k)
    merge_lists_device(_t(ids, np.int32), _t(sc, np.float32), _t(cnt, np.int32), o_i, o_s, o_c, 0, 0)
    p_i, p_s, p_c = _outs(B, k)
    merge_lists_packed_device(_packed(ids, sc, cnt), B, k, p_i, p_s, p_c, 0, 0)
    torch.cuda.synchronize()
    _check(o_i, o_s, o_c, exp, cnt, k, "lists")
    _check(p_i, p_s, p_c, exp, cnt, k, "packed")


def test_signed_zeros_and_ties_across_a_wide_merge():
    """2056 keys per query in random order: 20 x 0.25, 100 x +0.0, 100 x -0.0, the rest -0.25, so the best 257 hold every +0.0 ahead of every
    -0.0 whatever the ids, and equal bits by the larger id"""
    import cosdata_amd  # noqa: F401
    from cosdata_amd.sharding import merge_lists_device
    S, B, k = 8, 2, 257
    rng = np.random.default_rng(9)
    vals = np.concatenate([np.full(20, 0.25), np.full(100, 0.0), np.full(100, -0.0), np.full(S * k - 220, -0.25)]).astype(np.float32)
    sc = np.stack([rng.permutation(vals).reshape(S, k) for _ in range(B)], axis=1)
    ids = rng.permutation(S * B * k).astype(np.uint32).reshape(S, B, k)
    cnt = np.full((S, B), k, np.uint32)
    exp = _merge_numpy(ids, sc, cnt, k)
    assert (exp[1].view(np.uint32) == 0x80000000).any() and (exp[1].view(np.uint32) == 0).any()
    o_i, o_s, o_c = _outs(B, k)
    merge_lists_device(_t(ids, np.int32), _t(sc, np.float32), _t(cnt, np.int32), o_i, o_s, o_c, 0, 0)
    torch.cuda.synchronize()
    _check(o_i, o_s, o_c, exp, cnt, k, "zeros")


def test_more_than_8192_keys_are_refused_and_nothing_is_written():
    import cosdata_amd  # noqa: F401
    from cosdata_amd import _lib
    from cosdata_amd.sharding import merge_lists_device, merge_lists_packed_device
    rng = np.random.default_rng(4)
    for S, B, k in [(3, 2, 2731), (1, 1, 8193)]:
        ids, sc, cnt = _merge_inputs(rng, S, B, k, "full", "ties")
        o_i, o_s, o_c = _outs(B, k)
        with pytest.raises(_lib.CosdataError) as ei:
            merge_lists_device(_t(ids, np.int32), _t(sc, np.float32), _t(cnt, np.int32), o_i, o_s, o_c, 0, 0)
        assert ei.value.status == 4                      # COS_ERR_UNIMPLEMENTED
        with pytest.raises(_lib.CosdataError) as ei:
            merge_lists_packed_device(_packed(ids, sc, cnt), B, k, o_i, o_s, o_c, 0, 0)
        assert ei.value.status == 4
        torch.cuda.synchronize()
        assert (o_i == PAT_I).all() and (o_s == PAT_S).all() and (o_c == PAT_I).all()


@pytest.mark.parametrize("case", NARROW_SAME_BITS, ids=lambda c: "S%d-B%d-k%d" % c[:3])
def test_narrow_calls_return_the_bits_of_the_wave_kernel(case):
    """S * k <= 1024: whole output buffers (the untouched slots included) equal those of cos_merge_topk_device / _packed_device"""
    import cosdata_amd  # noqa: F401
    from cosdata_amd.sharding import merge_lists_device, merge_lists_packed_device, merge_topk_device, merge_topk_packed_device
    S, B, k, counts, scores = case
    rng = np.random.default_rng(S + B + k)
    ids, sc, cnt = _merge_inputs(rng, S, B, k, counts, scores)
    a, b, c, d = _outs(B, k), _outs(B, k), _outs(B, k), _outs(B, k)
    merge_topk_device(_t(ids, np.int32), _t(sc, np.float32), _t(cnt, np.int32), *a, 0, 0)
    merge_lists_device(_t(ids, np.int32), _t(sc, np.float32), _t(cnt, np.int32), *b, 0, 0)
    merge_topk_packed_device(_packed(ids, sc, cnt), B, k, *c, 0, 0)
    merge_lists_packed_device(_packed(ids, sc, cnt), B, k, *d, 0, 0)
    torch.cuda.synchronize()
    for x, y in ((a, b), (c, d), (a, d)):
        assert all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(x, y))
