"""The oracle's arithmetic at dimensions that are NOT a multiple of the vector widths (odd, below 16, one off a power of two):
the AVX2 tails of its dots, the final partial byte of a SubByte plane, the u8 rows that are no whole 16-byte chunk.  The GPU
tests hold the device to the oracle bit for bit at these dimensions (test_gpu_odd_dims.py); this file pins the oracle itself
against plain numpy restatements written from the reference's Rust (src/quantization/scalar.rs:10-52,
src/models/common.rs:226-275, src/distance/cosine.rs:223-235, src/distance/dot_product.rs), sharing no code with
cosdata_oracle_num.c."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import odd_dims as OD
from tests.odd_dims import D, STORAGES, U


def special_rows(n, dim, seed, amp=1.3):
    """uniform rows carrying the quirk values of test_quantize_matches_oracle (1.0 wraps / saturates, -1.0, NaN, 5e30) at
    positions that exist at every dim >= 1 (first, last and middle element), and an all-zero row"""
    x = np.random.default_rng(seed).uniform(-amp, amp, (n, dim)).astype(np.float32)
    sp = np.array([1.0, -1.0, np.nan, 5e30], np.float32)
    x[0, :min(4, dim)] = sp[:min(4, dim)]
    x[1, :] = 0.0
    x[2, 0], x[3, 0], x[4, dim - 1], x[5, dim // 2], x[6, dim - 1] = sp[0], sp[1], sp[2], sp[3], sp[0]
    return x


def seq_norm_np(x):
    """sqrt of the sequential, non-fused f32 sum of x*x (scalar.rs:31-32,41,45).  <f32 as Sum> folds from -0.0, the additive
    identity, so the first square enters unchanged: the running sum IS np.add.accumulate."""
    sq = x * x
    return np.sqrt(np.add.accumulate(sq, axis=1, dtype=np.float32)[:, -1])


def usize_low_bits(t, res):
    """low `res` bits of `t as usize` for an f32 t (Rust's saturating cast: NaN and negatives -> 0, >= 2^64 -> usize::MAX)"""
    mask = (1 << res) - 1
    out = np.zeros(t.shape, np.uint8)
    small = (t > 0) & (t < 2.0 ** 32)                   # from 2^27 up an f32 is a multiple of 16: the low 3 bits are 0
    out[small] = (t[small].astype(np.uint64) & np.uint64(mask)).astype(np.uint8)
    out[t >= 2.0 ** 64] = mask
    return out


def quantize_np(x, storage, res, lo=-1.0, hi=1.0):
    """-> (codes uint8 [n, code_bytes], mags f32 [n]) in the reference's layout: SubByte is plane-major, plane p holding bit
    res-1-p of the level (to_float_flag fills from the least significant bit backwards), dimension i at bit i % 8 of byte i / 8"""
    n, dim = x.shape
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        if storage == O.STORAGE_U8:
            c = np.fmin(np.fmax(x, lo), hi)              # f32::max / min return the other operand for a NaN
            v = ((c - lo) / (hi - lo)) * np.float32(255.0)
            q = v.astype(np.uint8)                       # v is in [0, 255]: `as u8` truncates
            s = (q.astype(np.uint32) * q.astype(np.uint32)).sum(axis=1, dtype=np.uint32)
            return q, np.sqrt(s.astype(np.float32))
        if storage == O.STORAGE_SUBBYTE:
            step = np.float32(2.0) / np.float32(1 << res)
            level = usize_low_bits(np.floor((x + np.float32(1.0)) / step), res)
            pb = (dim + 7) // 8
            codes = np.zeros((n, res, pb), np.uint8)
            for p in range(res):
                bit = (level >> (res - 1 - p)) & 1
                padded = np.zeros((n, pb * 8), np.uint8)
                padded[:, :dim] = bit
                codes[:, p, :] = np.packbits(padded.reshape(n, pb, 8), axis=2, bitorder="little")[:, :, 0]
            return codes.reshape(n, res * pb), seq_norm_np(x)
        if storage == O.STORAGE_F16:
            return np.ascontiguousarray(x.astype(np.float16)).view(np.uint8).reshape(n, dim * 2), seq_norm_np(x)
        return np.ascontiguousarray(x).view(np.uint8).reshape(n, dim * 4), seq_norm_np(x)


@pytest.mark.parametrize("name,storage,res", STORAGES)
@pytest.mark.parametrize("dim", D)
def test_quantize_equals_numpy_restatement(name, storage, res, dim):
    x = special_rows(37, dim, seed=dim)
    codes, mags = O.quantize_batch(x, storage, res, -1.0, 1.0)
    ncodes, nmags = quantize_np(x, storage, res)
    assert codes.shape == ncodes.shape
    assert np.array_equal(codes, ncodes)
    assert np.array_equal(mags.view(np.uint32), nmags.view(np.uint32))
    if storage == O.STORAGE_SUBBYTE and dim % 8:
        last = codes.reshape(37, res, -1)[:, :, -1]
        assert not (last >> (dim % 8)).any(), "bits past dim in the final partial byte of a plane"
        assert (last & ((1 << (dim % 8)) - 1)).any(), "the final partial byte carries no dimension at all"


def digits(codes, storage, res, dim):
    """the integers the reference multiplies: u8 bytes, or per dimension sum_p 2^p * (bit of STORED plane p) — plane 0, which
    holds the level's most significant bit, is multiplied as the least significant one (dot_product.rs:35-57, 64-90)"""
    if storage == O.STORAGE_U8:
        return codes.astype(np.int64)
    n = codes.shape[0]
    planes = np.unpackbits(codes.reshape(n, res, -1), axis=2, bitorder="little")[:, :, :dim].astype(np.int64)
    return sum(planes[:, p, :] << p for p in range(res))


@pytest.mark.parametrize("name,storage,res", STORAGES[:4])
@pytest.mark.parametrize("dim", D)
def test_integer_distance_equals_exact_dot(name, storage, res, dim):
    """cosine = (dot as f32) / (x_mag * y_mag) with one f32 multiply and one divide (cosine.rs:228-233); DotProduct = dot as f32.
    The integer dot is exact, so both are asserted bit for bit; a zero denominator is CalculationError."""
    x = np.random.default_rng(1000 + dim).uniform(-1.2, 1.2, (14, dim)).astype(np.float32)
    x[3] = 0.0                                           # SubByte: mag 0
    x[4] = -1.0                                          # u8: all-zero code, mag 0
    codes, mags = O.quantize_batch(x, storage, res, -1.0, 1.0)
    dg = digits(codes, storage, res, dim)
    dots = dg @ dg.T
    n_err = 0
    for i in range(14):
        for j in range(14):
            fdot = np.float32(int(dots[i, j]))           # u64 as f32: round to nearest even
            rc, v = O.distance(O.METRIC_DOT, storage, res, dim, codes[i], mags[i], codes[j], mags[j])
            assert rc == O.OK and v.tobytes() == fdot.tobytes(), (i, j, v, fdot)
            den = np.float32(mags[i]) * np.float32(mags[j])
            rc, v = O.distance(O.METRIC_COSINE, storage, res, dim, codes[i], mags[i], codes[j], mags[j])
            if den == 0.0:
                assert rc == 2, (i, j, rc)
                n_err += 1
            else:
                assert rc == O.OK and v.tobytes() == (fdot / den).tobytes(), (i, j, v, fdot / den)
    assert n_err >= 27                                   # the zero-norm row against every row, both ways


@pytest.mark.parametrize("name,storage,res", STORAGES[4:])
@pytest.mark.parametrize("dim", D)
def test_float_distance_within_derived_bound(name, storage, res, dim):
    """f32: the 8-chain FMA dot + pairwise tree + scalar tail (x86_64.rs:418-444) over two norms and a divide:
    |s - cos64| <= (dim/8 + 16) u * sum|x_i y_i| / (|x||y|) + 4u, u = 2^-24.
    f16 is held to the SAME bound.  What changes is the value it approaches: the float64 dot of the DECODED f16 values over the
    float64 norms of the original vectors (scalar.rs:39-42: the code is rounded, the magnitude is not).  Its products are exact in
    f32 (two 11-bit significands) and are summed sequentially (dot_product.rs:13-19)."""
    x = np.random.default_rng(2000 + dim).uniform(-1.0, 1.0, (14, dim)).astype(np.float32)
    x[3] = 0.0
    codes, mags = O.quantize_batch(x, storage, res, -1.0, 1.0)
    if storage == O.STORAGE_F16:
        dec = np.ascontiguousarray(codes).view(np.float16).astype(np.float64)
    else:
        dec = x.astype(np.float64)
    k = dim / 8 + 16
    norm = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    worst = 0.0
    for i in range(14):
        for j in range(14):
            rc, v = O.distance(O.METRIC_COSINE, storage, res, dim, codes[i], mags[i], codes[j], mags[j])
            if i == 3 or j == 3:
                assert rc == 2
                continue
            den = norm[i] * norm[j]
            cos64 = float(dec[i] @ dec[j]) / den
            bound = k * U * float(np.abs(dec[i] * dec[j]).sum()) / den + 4 * U
            err = abs(float(v) - cos64)
            worst = max(worst, err / bound)
            assert rc == O.OK and err <= bound, (i, j, float(v), cos64, err, bound)
    print(f"{name} dim {dim}: worst error / bound = {worst:.3f}")


# ---- the second opinion, confirmed on the oracle alone before the device is held to it (test_gpu_odd_dims.py asserts the same
# ---- of the device on the same corpora) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,B,k", OD.BRUTE_CASES + [OD.BRUTE_BORROWED])
def test_oracle_bruteforce_is_the_float64_topk(n, dim, B, k):
    X, Q = OD.brute_corpus(n, dim, B)
    ids, sc = O.bruteforce_topk(X, Q, k, threads=8)
    worst = OD.assert_scores_within_bound(X, Q, ids, sc, what="bruteforce")
    excused = OD.float64_topk_excused(X, Q, ids, k)
    print(f"n {n} dim {dim}: worst error / bound {worst:.3f}, {excused} of {B} queries excused")
    assert excused <= 0.05 * B


@pytest.mark.parametrize("name,storage,res", [s for s in STORAGES if s[0] in ("u8", "f16", "f32")])
def test_oracle_rerank_scores_are_the_float64_cosine(name, storage, res):
    worst = 0.0
    for dim in OD.WALK_DIMS:
        for kind in ("uniform", "clustered"):
            X = OD.walk_corpus(kind, 600, dim, storage)
            Q = OD.walk_queries(X, dim, storage)
            p = O.HNSWParams(dim=dim, storage=storage, resolution=res, num_layers=3, ef_construction=24, ef_search=32)
            ids, sc, cnt = O.OracleIndex(p).set_vectors(X).build().search_batch(Q, 10, threads=4)[:3]
            worst = max(worst, OD.assert_scores_within_bound(X, Q, ids, sc, cnt, what=f"{name} dim {dim} {kind}"))
    print(f"{name}: worst error / bound {worst:.3f}")
