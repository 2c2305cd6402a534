"""The host models behind the device check of the latency kernels' evaluation blocks (tests/cxx/lat_dots_host.h, run by
tests/cxx/lat_dots_selftest.cpp on a CPU) are the oracle's, and the generated inputs tell the reference order from wrong ones.

Every dot the self-test prints equals O.dot_f32 / O.dot_f16 / O.dot_subbyte on the same inputs in bits (a NaN: NaN on both sides, same
sign), every parked word is what O.distance answers under cosine and dot product (CalculationError <=> bit 32), and every finite float
dot lies inside the forward error bound of any summation order, gamma_n * sum|x_i * y_i| around the float64 dot — a derived bound on
model and oracle alike, not a tolerance on a kernel.

Share of the (query, row) pairs with finite products (non-zero query, no inf / NaN row) that each wrong order changes, over the dims at
which it is another computation at all (lat_dots_host.h f32_variant_applies / f16_variant_applies), and the smallest share at one dim:
    f32  one sequential chain   62.7 %  (least 14.7 % at dim 15)
    f32  unfused chain steps    31.4 %  (least  9.5 % at dim 71)
    f32  fused tail             27.1 %  (least  3.2 % at dim 17: 6 of 190 pairs)
    f32  tree as a left fold    36.9 %  (least 13.2 % at dim 71)
    f16  eight chains           75.8 %  (least 29.9 % at dim 7)
    f16  +0.0 start             differs exactly on the all-negative row against the zero query (-0.0 against +0.0), at every dim
    f16  fused steps            0 by arithmetic: a product of two f16 values is exact in f32, so the fused step rounds the same number;
                                the self-test asserts the equality instead
"""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")
F32, F16, BIN, OCT = 0, 1, 2, 3  # lat_dots_host.h Storage
ORACLE_STORAGE = {F32: (O.STORAGE_F32, 0), F16: (O.STORAGE_F16, 0), BIN: (O.STORAGE_SUBBYTE, 1), OCT: (O.STORAGE_SUBBYTE, 3)}
ZERO_QUERY, ZERO_ROW = 2, 3
SUBNORMAL, PINF, NINF, NAN, NZERO, MAX, NEG = 8, 9, 10, 11, 12, 13, 14  # the special f16 rows
F32_VARIANTS = ("one_chain", "unfused_steps", "fused_tail", "left_fold")
F16_VARIANTS = ("plus_zero_start", "fused_steps", "eight_chains")


def _f32_applies(v, n):
    steps, tail = n // 8, n % 8
    return {"one_chain": steps >= 1, "left_fold": steps >= 1, "unfused_steps": steps >= 2, "fused_tail": tail >= 2 or (tail >= 1 and steps >= 1)}[v]


def _f16_applies(v, n):
    return {"plus_zero_start": n >= 1, "eight_chains": n >= 4, "fused_steps": False}[v]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """{(storage, dim): dict(q=codes [3][..], rows=codes [96][..], out={(query, row): (dot, qmag, mag, word_cos, word_dot, variants)})}"""
    tmp = tmp_path_factory.mktemp("lat_dots")
    exe, dump = tmp / "lat_dots_selftest", tmp / "inputs.bin"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(CXX, "lat_dots_selftest.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(dump)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    buf, off, m = np.fromfile(dump, np.uint8), 0, {}
    while off < buf.size:
        st, dim, nq, nrows, nbytes = (int(v) for v in buf[off:off + 20].view(np.int32))
        off += 20
        q = buf[off:off + nq * nbytes].reshape(nq, nbytes)
        off += nq * nbytes
        rows = buf[off:off + nrows * nbytes].reshape(nrows, nbytes)
        off += nrows * nbytes
        m[(st, dim)] = dict(q=q, rows=rows, out={})
    for line in r.stdout.splitlines():
        t = line.split()
        assert t[0] == "D"
        st, dim, qi, row = (int(v) for v in t[1:5])
        m[(st, dim)]["out"][(qi, row)] = tuple(int(v, 16) for v in t[5:10]) + (tuple(int(v, 16) for v in t[10:]),)
    assert len(m) == 24 + 17 + 9 + 9 and all(len(v["out"]) == 3 * 96 for v in m.values())
    return m


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _same_f32(a, b):
    an, bn = (a & 0x7FFFFFFF) > 0x7F800000, (b & 0x7FFFFFFF) > 0x7F800000
    if an or bn:
        return an and bn and (a >> 31) == (b >> 31)
    return a == b


def _key_value_bits(key):  # metric_key_inv for the metrics that do not complement
    return key ^ 0x80000000 if key & 0x80000000 else ~key & 0xFFFFFFFF


def _as_f32(u):
    return np.array([u], np.uint32).view(np.float32)[0]


def _oracle_dot(st, q, row):
    if st == F32:
        return _bits(O.dot_f32(q.view(np.float32), row.view(np.float32)))
    if st == F16:
        return _bits(O.dot_f16(q.view(np.uint16), row.view(np.uint16)))
    v, status = O.dot_subbyte(q, row, ORACLE_STORAGE[st][1])
    assert status == O.OK
    return _bits(v)


def test_model_dots_and_parked_words_are_the_oracles(model):
    n = 0
    for (st, dim), m in model.items():
        storage, res = ORACLE_STORAGE[st]
        for (qi, ri), (dot, qmag, mag, wcos, wdot, _) in m["out"].items():
            q, row = m["q"][qi], m["rows"][ri]
            where = (st, dim, qi, ri)
            assert _same_f32(dot, _oracle_dot(st, q, row)), where
            rc, v = O.distance(O.METRIC_COSINE, storage, res, dim, q, _as_f32(qmag), row, _as_f32(mag))
            assert (rc == O.ERR_CALCULATION) == bool(wcos >> 32) and rc in (O.OK, O.ERR_CALCULATION), where
            assert bool(wcos >> 32) == (qi == ZERO_QUERY or ri == ZERO_ROW), where
            if rc == O.OK:
                assert _same_f32(_key_value_bits(wcos & 0xFFFFFFFF), _bits(v)), where
            rc, v = O.distance(O.METRIC_DOT, storage, res, dim, q, _as_f32(qmag), row, _as_f32(mag))
            assert wdot >> 32 == 0, where
            if st == F32:  # DotProductDistance has no f32 arm: the word is the dot itself
                assert rc == O.ERR_STORAGE_MISMATCH and _same_f32(_key_value_bits(wdot), dot), where
            else:
                assert rc == O.OK and _same_f32(_key_value_bits(wdot), _bits(v)), where
            n += 1
    assert n == 59 * 3 * 96


def _widened(st, codes):
    return codes.view(np.float32).astype(np.float64) if st == F32 else codes.view(np.uint16).view(np.float16).astype(np.float64)


def test_float_dots_lie_inside_the_forward_error_bound_of_any_order(model):
    n = 0
    for (st, dim), m in model.items():
        if st not in (F32, F16):
            continue
        Q, X = _widened(st, m["q"]), _widened(st, m["rows"])
        with np.errstate(invalid="ignore", over="ignore"):
            exact, mass = Q @ X.T, np.abs(Q) @ np.abs(X).T
        gamma = dim * 2.0 ** -24 / (1.0 - dim * 2.0 ** -24)
        for (qi, ri), out in m["out"].items():
            if not np.isfinite(mass[qi, ri]):
                continue
            got = float(_as_f32(out[0]))
            assert abs(got - exact[qi, ri]) <= gamma * mass[qi, ri], (st, dim, qi, ri, got, exact[qi, ri])
            n += 1
    assert n > 10000


def _shares(model, st, names, applies):
    """per variant: (changed, pairs) over all applicable dims, and the smallest share at one dim with the dim"""
    total, worst = {v: [0, 0] for v in names}, {v: (2.0, None) for v in names}
    for (s, dim), m in model.items():
        if s != st:
            continue
        finite = np.isfinite(_widened(st, m["rows"])).all(axis=1)
        for k, v in enumerate(names):
            if not applies(v, dim):
                continue
            pairs = [(key, out) for key, out in m["out"].items() if key[0] != ZERO_QUERY and key[1] != ZERO_ROW and finite[key[1]]]
            changed = sum(out[5][k] != out[0] for _, out in pairs)
            total[v][0] += changed
            total[v][1] += len(pairs)
            if changed / len(pairs) < worst[v][0]:
                worst[v] = (changed / len(pairs), dim)
    return total, worst


def test_f32_inputs_tell_the_reference_order_from_wrong_ones(model):
    total, worst = _shares(model, F32, F32_VARIANTS, _f32_applies)
    for v in F32_VARIANTS:
        print(f"f32 {v}: {total[v][0]} of {total[v][1]} pairs change ({100.0 * total[v][0] / total[v][1]:.1f} %), least {100.0 * worst[v][0]:.1f} % at dim {worst[v][1]}")
        assert worst[v][0] > 0.0, (v, worst[v])  # at EVERY dim where the variant is another computation some row shows it
    for (s, dim), m in model.items():  # ... and where it is not, it is the same number
        for k, v in enumerate(F32_VARIANTS):
            if s == F32 and not _f32_applies(v, dim):
                assert all(out[5][k] == out[0] for out in m["out"].values()), (v, dim)


def test_f16_inputs_tell_the_reference_order_from_wrong_ones(model):
    total, worst = _shares(model, F16, F16_VARIANTS, _f16_applies)
    v = "eight_chains"
    print(f"f16 {v}: {total[v][0]} of {total[v][1]} pairs change ({100.0 * total[v][0] / total[v][1]:.1f} %), least {100.0 * worst[v][0]:.1f} % at dim {worst[v][1]}")
    assert worst[v][0] > 0.0, worst[v]
    for (s, dim), m in model.items():
        if s != F16:
            continue
        dot, _, _, _, _, var = m["out"][(ZERO_QUERY, NEG)]  # every product is -0.0: the chain stays at -0.0, a +0.0 start does not
        assert dot == 0x80000000 and var[0] == 0x00000000, dim
        assert all(_same_f32(out[5][1], out[0]) for out in m["out"].values()), dim  # fused steps: the same number (exact products)


def test_f16_rows_carry_every_special_code_in_first_middle_and_last_tile(model):
    kinds = {SUBNORMAL: lambda h: ((h & 0x7C00) == 0) & ((h & 0x3FF) != 0), PINF: lambda h: h == 0x7C00, NINF: lambda h: h == 0xFC00,
             NAN: lambda h: ((h & 0x7C00) == 0x7C00) & ((h & 0x3FF) != 0), NZERO: lambda h: h == 0x8000, MAX: lambda h: (h & 0x7FFF) == 0x7BFF}
    for (st, dim), m in model.items():
        if st != F16:
            continue
        for row, is_kind in kinds.items():
            at = np.flatnonzero(is_kind(m["rows"][row].view(np.uint16)))
            for td in (64, 128):
                nt = (dim + td - 1) // td
                assert {0, nt // 2, nt - 1} <= set(at // td), (dim, row, td)
        h = m["rows"][NEG].view(np.uint16)
        assert np.all(h & 0x8000) and not np.any(m["q"][ZERO_QUERY])
