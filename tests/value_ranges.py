"""The `values_range` cases of the dense u8 paths, shared by test_oracle_value_ranges.py (no device) and test_gpu_value_ranges.py.

The range decides every code byte: ((x.max(lo).min(hi) - lo) / (hi - lo)) * 255.0) as u8 (scalar.rs:21-22).  Under the default
(-1, 1) the divisor is exactly 2.0, L2-normalised rows use 105 of the 256 code values and none of them is 0 or 255; "auto"
quantization (sample_values_range) and every range the sampler can return look different: all 256 values, saturated codes, a
division that rounds.  This module holds the ranges, the input that makes a wrongly rounded division visible (ladder), a restatement
of the quantizer that shares no code with the oracle or the kernel (quantize_u8_numpy), and the corpora and queries of the device
tests, so that the CPU test can assert what those inputs contain."""
import numpy as np

from oracle import oracle as O
from tests import helpers as H

F = np.float32


def f32_range(lo, hi):
    """(lo, hi) as Python floats that hold f32 values exactly: the device and the oracle get the same bits"""
    return float(F(lo)), float(F(hi))


RANGES = [(name,) + f32_range(lo, hi) for name, lo, hi in [("tight", -0.025, 0.025), ("asym_low", -0.025, 0.3), ("asym_high", -0.5, 0.05)]]
DEGENERATE = [("lo_equals_hi", ) + f32_range(0.1, 0.1), ("lo_above_hi", ) + f32_range(0.3, -0.025)]
SYMMETRIC = [("pm0.1",) + f32_range(-0.1, 0.1), ("pm0.3",) + f32_range(-0.3, 0.3), ("default",) + f32_range(-1.0, 1.0)]


def sampled(X):
    """the benchmark's rule: quantization = "auto" """
    return f32_range(*O.sample_values_range(np.ascontiguousarray(X[:1000]), 1.0))


def ranges_for(X, names=("sampled", "tight", "asym_low", "asym_high")):
    table = {name: (lo, hi) for name, lo, hi in RANGES}
    return [(name, *(sampled(X) if name == "sampled" else table[name])) for name in names]


# ---- the quantizer's input -------------------------------------------------------------------------------------------------------
LADDER_STEPS = 256 * 7


def ladder(lo, hi):
    """the 256 values at which the quotient sits on an integer, lo + k/255 * (hi - lo) (f64 from the f32 bounds, rounded to f32), each
    with its three f32 neighbours on either side: the first LADDER_STEPS entries.  `as u8` truncates, so a division that is one ulp
    off changes a byte only there.  Then the specials: the bounds and their neighbours outside the range, +-0.0, the smallest
    subnormal and the largest finite float with both signs, +-inf, NaN."""
    lo, hi = F(lo), F(hi)
    steps = (np.float64(lo) + np.arange(256, dtype=np.float64) / 255.0 * (np.float64(hi) - np.float64(lo))).astype(F)
    cols = [steps]
    down = up = steps
    for _ in range(3):
        down, up = np.nextafter(down, F(-np.inf)), np.nextafter(up, F(np.inf))
        cols += [down, up]
    body = np.sort(np.stack(cols, axis=1), axis=1).ravel()
    tiny, huge = F(np.nextafter(F(0), F(1))), np.finfo(F).max
    outer = [lo, hi, np.nextafter(min(lo, hi), F(-np.inf)), np.nextafter(max(lo, hi), F(np.inf))]
    specials = np.array(outer + [0.0, -0.0, tiny, -tiny, huge, -huge, np.inf, -np.inf, np.nan], F)
    out = np.concatenate([body, specials]).astype(F)
    assert body.size == LADDER_STEPS
    return out


def ladder_rows(lo, hi, width):
    """the ladder as rows of `width` values; the last row is filled up with NaN (which quantizes to the code of lo)"""
    x = ladder(lo, hi)
    rows = -(-x.size // width)
    out = np.full(rows * width, np.nan, F)
    out[:x.size] = x
    return out.reshape(rows, width)


def quantize_u8_numpy(x, lo, hi, division="divide"):
    """scalar.rs:21-22 in f32 numpy -> codes [.. same shape ..] u8.  `division`: "divide" is the reference's; "reciprocal" multiplies
    by 1 / (hi - lo) and "folded" by 255 / (hi - lo): the two cheaper forms a kernel could take, wrong by one ulp in places"""
    x, lo, hi = np.asarray(x, F), F(lo), F(hi)
    with np.errstate(all="ignore"):
        c = np.where(np.isnan(x), lo, np.maximum(x, lo))              # f32::max: a NaN operand loses
        c = np.minimum(c, hi).astype(F)                               # (c is never NaN here)
        num, den = (c - lo).astype(F), F(hi - lo)
        if division == "divide":
            v = ((num / den).astype(F) * F(255.0)).astype(F)
        elif division == "reciprocal":
            v = ((num * F(F(1.0) / den)).astype(F) * F(255.0)).astype(F)
        elif division == "folded":
            v = (num * F(F(255.0) / den)).astype(F)
        else:
            raise ValueError(division)
        q = np.zeros(v.shape, np.uint8)                               # `as u8`: NaN and everything <= 0 -> 0
        q[v >= F(255.0)] = 255
        mid = (v > 0) & (v < F(255.0))
        q[mid] = np.trunc(v[mid]).astype(np.uint8)
    return q


def mags_u8_numpy(codes):
    """(sum::<u32>(q * q) as f32).sqrt() per row"""
    s = (codes.astype(np.uint64) ** 2).sum(axis=-1) & 0xFFFFFFFF
    return np.sqrt(s.astype(F)).astype(F)


# ---- the corpora and queries of the device tests -----------------------------------------------------------------------------------
_cache = {}


def corpus(n, dim, seed=0):
    """H.clustered_corpus with one component in 256 made an outlier (six times its value, as embedding models' outlier dimensions are):
    L2-normalised rows alone never reach -0.5 at 96 dims or +-0.3 at 1024, and every range must see both saturated codes"""
    key = ("corpus", n, dim, seed)
    if key not in _cache:
        X = H.clustered_corpus(n, dim, n_centers=24, seed=1700 + seed + dim)
        out = np.random.default_rng(seed + 5).random(X.shape) < 1.0 / 256.0
        X = np.where(out, X * F(6.0), X).astype(F)
        X.setflags(write=False)
        _cache[key] = X
    return _cache[key]


def walk_queries(X, lo, n_near=24, n_uniform=8):
    """queries near corpus rows, uniform ones, and one planted at range_lo as the LAST row: the all-zero code, |q| = 0"""
    dim = X.shape[1]
    Q = np.concatenate([H.queries_from(X, n_near, seed=3), H.uniform_corpus(n_uniform, dim, seed=99), np.full((1, dim), lo, F)])
    return np.ascontiguousarray(Q.astype(F))


def scan_queries(X, B, seed=8):
    """B queries for the exhaustive scans: B - 2 near corpus rows, two uniform; none with a zero norm"""
    return np.ascontiguousarray(np.concatenate([H.queries_from(X, B - 2, noise=0.05, seed=seed), H.uniform_corpus(2, X.shape[1], seed=77)]))


# (name, n, dim, range names): every corpus of test_gpu_value_ranges.py, for the input conditions asserted without a device
ALL = ("sampled", "tight", "asym_low", "asym_high")
WORLDS = [
    ("codes", 300, 100, ALL),
    ("walk", 2000, 96, ALL),
    ("walk", 1500, 100, ALL),
    ("table", 4000, 128, ("sampled", "tight")),
    ("table", 3000, 1024, ("sampled", "tight")),
    ("flat", 3001, 100, ALL),
    ("fused", 16500, 128, ALL),
    ("fused", 16500, 1024, ALL),
    ("builder", 1800, 96, ("sampled", "asym_low")),
    ("shards", 3000, 96, ("asym_high",)),
]


WALKED = ("walk", "table", "builder")          # worlds whose queries go through the graph: the last one is planted at range_lo


def world(name, n, dim):
    return corpus(n, dim, seed=sum(map(ord, name)))


def queries(name, X, lo):
    """the queries the device tests of world `name` send under a range that starts at `lo`; the table GEMM gets a second 64-row block"""
    if name in WALKED:
        return walk_queries(X, lo, n_near=64 if name == "table" else 24)
    return scan_queries(X, {"fused": 40, "shards": 9}.get(name, 5))
