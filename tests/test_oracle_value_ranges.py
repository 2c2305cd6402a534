"""CPU: the oracle's u8 quantizer under the ranges the sampler can return, against an f32 numpy restatement of scalar.rs:21-22 that
shares no code with it (tests/value_ranges.py), on the input where a wrongly rounded division shows (the ladder); and the input
conditions of test_gpu_value_ranges.py, asserted here so that the device tests cannot pass on inputs that hold nothing."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import value_ranges as VR

CASES = VR.RANGES + VR.SYMMETRIC + VR.DEGENERATE


@pytest.mark.parametrize("name,lo,hi", CASES, ids=[c[0] for c in CASES])
def test_oracle_quantizer_equals_the_numpy_restatement_on_the_ladder(name, lo, hi):
    x = VR.ladder(lo, hi)
    assert x.size == VR.LADDER_STEPS + 13 and np.isnan(x).sum() == 1 and np.isinf(x).sum() == 2
    codes, mags = O.quantize_batch(x[None, :], O.STORAGE_U8, 0, lo, hi)
    want = VR.quantize_u8_numpy(x, lo, hi)
    assert np.array_equal(codes[0], want), np.flatnonzero(codes[0] != want)
    assert np.array_equal(mags.view(np.uint32), VR.mags_u8_numpy(want[None, :]).view(np.uint32))
    if lo >= hi:
        assert set(np.unique(want)) <= {0, 255}
    # the specials, one by one: the NaN -> lo rule and the saturation, which random corpora never reach
    sp = dict(zip(["lo", "hi", "below", "above", "+0", "-0", "+tiny", "-tiny", "+huge", "-huge", "+inf", "-inf", "nan"], codes[0][VR.LADDER_STEPS:]))
    if lo < hi:
        assert sp["lo"] == sp["below"] == sp["-huge"] == sp["-inf"] == sp["nan"] == 0
        assert sp["hi"] == sp["above"] == sp["+huge"] == sp["+inf"] == 255
        assert sp["+0"] == sp["-0"] == sp["+tiny"] == sp["-tiny"]
    elif lo == hi:
        assert set(sp.values()) == {0}                                   # 0 / 0 = NaN -> 0
    else:
        assert set(sp.values()) == {255}                                 # everything clamps to hi: (hi - lo) / (hi - lo) = 1


def test_rows_of_every_width_quantize_like_one_long_row():
    """the oracle's batch call row by row equals the restatement on the reshaped ladder, mags included (dims 1 .. 100)"""
    _, lo, hi = VR.RANGES[1]
    for width in (1, 15, 16, 17, 64, 100):
        x = VR.ladder_rows(lo, hi, width)
        codes, mags = O.quantize_batch(x, O.STORAGE_U8, 0, lo, hi)
        want = VR.quantize_u8_numpy(x, lo, hi)
        assert np.array_equal(codes, want), width
        assert np.array_equal(mags.view(np.uint32), VR.mags_u8_numpy(want).view(np.uint32)), width


@pytest.mark.parametrize("name,lo,hi", VR.RANGES, ids=[c[0] for c in VR.RANGES])
def test_the_ladder_tells_a_cheaper_division_from_the_reference(name, lo, hi):
    """why the ladder exists: multiplying by a reciprocal, or by a folded 255 / (hi - lo), changes bytes on it under every range of
    RANGES, and none under (-1, 1), where the divisor is 2.0 and every form is exact"""
    x = VR.ladder(lo, hi)[:VR.LADDER_STEPS]
    ref = VR.quantize_u8_numpy(x, lo, hi)
    d1 = VR.ladder(-1.0, 1.0)[:VR.LADDER_STEPS]
    for form in ("reciprocal", "folded"):
        diff = int(np.count_nonzero(VR.quantize_u8_numpy(x, lo, hi, form) != ref))
        print(f"{name}: {form} changes {diff} of {x.size} bytes")
        assert diff > 0, form
        assert np.array_equal(VR.quantize_u8_numpy(d1, -1.0, 1.0, form), VR.quantize_u8_numpy(d1, -1.0, 1.0)), form


def _conditions(X, Q, planted, name, lo, hi, what):
    codes, mags = O.quantize_batch(X, O.STORAGE_U8, 0, lo, hi)
    assert (mags > 0).all(), (what, name, "a stored row has zero norm")
    _, qmags = O.quantize_batch(Q, O.STORAGE_U8, 0, lo, hi)
    assert sorted(np.flatnonzero(qmags == 0)) == sorted(planted), (what, name, np.flatnonzero(qmags == 0))
    hist = np.bincount(codes.ravel(), minlength=256)
    assert hist[0] > 0 and hist[255] > 0, (what, name, hist[0], hist[255])
    share = (hist[0] + hist[255]) / codes.size
    if name in ("tight", "asym_low"):
        assert share >= 0.2, (what, name, share)
    return share, int(np.count_nonzero(hist))


@pytest.mark.parametrize("what,n,dim,names", VR.WORLDS, ids=[f"{w[0]}-{w[1]}x{w[2]}" for w in VR.WORLDS])
def test_input_conditions_of_the_device_worlds(what, n, dim, names):
    X = VR.world(what, n, dim)
    if dim == 1024 and n > 4000:
        X = X[:4000]                                                     # (rows are i.i.d.: a slice shows the same, a 17 M-value quantize loop does not fit a quick test)
    assert VR.sampled(X) != (-1.0, 1.0) and VR.sampled(X) == VR.sampled(VR.world(what, n, dim))
    for name, lo, hi in VR.ranges_for(X, names):
        Q = VR.queries(what, X, lo)
        planted = [Q.shape[0] - 1] if what in VR.WALKED else []
        share, distinct = _conditions(X, Q, planted, name, lo, hi, what)
        print(f"{what} {n} x {dim} {name} ({lo}, {hi}): {distinct} code values, share of 0 / 255 {share:.3f}")


@pytest.mark.parametrize("dim", [128, 1000])
def test_input_conditions_of_the_pair_walk_world(dim):
    """test_gpu_walk_pair's corpus under `tight`, the cases test_gpu_value_ranges.py adds"""
    from tests import test_gpu_walk_pair as WP
    _, lo, hi = VR.RANGES[0]
    X = WP._corpus(dim)
    Q = WP._make_queries(X, dim, 64, lo)
    share, distinct = _conditions(X[:3000], Q, [150], "tight", lo, hi, "pair")
    print(f"pair {dim}: {distinct} code values, share of 0 / 255 {share:.3f}")
    assert distinct == 256
