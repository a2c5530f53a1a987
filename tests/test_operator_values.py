"""The oracle's operator values (oracle/sr_oracle_ops.h) against the independent fixture
tests/golden/operators.npz (exact rational arithmetic and mpmath at 80 digits;
tests/golden/make_operator_golden.py), on the CPU.

The engine is held to the same fixture in every kernel family by
tests/test_operator_values_gpu.py; this file keeps the fixture honest (it loads, every
point has a finite bound, it is what its generator says) and pins the oracle to it:
within `oracle_err_ulp` at every point, bit-identical to RN_T(true value) for the exact
operators, and in agreement with every hand-written failure and convention entry.
"""
import numpy as np
import pytest

import operator_cases as C

TIDS = dict(ids=lambda T: np.dtype(T).name)


def test_the_fixture_covers_every_operator():
    """29 unary and 11 binary operators, each with a grid of at most 256 points (a block, for the binary ones)
    in both dtypes, and a finite bound at every point."""
    from srhip import constants as K

    assert {n.lower() for n in K.UOPS} == set(C.unary_ops()) and len(C.unary_ops()) == 29
    assert len(C.binary_ops()) == len(K.BOPS) == 11
    gen = C.generator()
    assert gen.MAX_POINTS == 256 and (gen.BAR_TRANS, gen.BAR_GAMMA) == (4.0, 16.0)
    exact = {op for op in C.unary_ops() + C.binary_ops() if C.is_exact(op)}
    assert exact == {"+", "-", "*", "/", "neg", "abs", "square", "cube", "sqrt", "relu", "round", "floor", "ceil", "sign",
                     "inv", "max", "min", "mod", "greater", "logical_or", "logical_and"}
    seen = 0
    for T in C.DTYPES:
        for op in C.unary_ops():
            c = C.unary_case(op, T)
            assert 10 <= len(c["x"]) <= 256, (op, len(c["x"]))
            assert np.array_equal(c["x"].astype(T).astype(np.float64), c["x"]), op  # operands exact in T
            with np.errstate(over="ignore"):
                assert np.isfinite(c["hi"].astype(T)).all(), op  # every value finite in T
            assert np.isfinite(C.bound(op, T, c["hi"])).all() and np.isfinite(c["lo"]).all(), op
            assert C.bar_ulp(op, T) == (0.0 if op in exact else 16.0 if op == "gamma" else 4.0)
            seen += len(c["x"])
        for op in C.binary_ops():
            for blk in C.binary_blocks(op, T):
                assert len(blk["x"]) == len(blk["a"]) * len(blk["b"]) <= 256, op
                with np.errstate(over="ignore"):
                    assert np.isfinite(blk["hi"].astype(T)).all(), op
                assert np.isfinite(C.bound(op, T, blk["hi"])).all()
                seen += len(blk["x"])
    assert seen > 10000
    assert (C.GOLDEN / "operators.npz").stat().st_size <= (C.GOLDEN / "derivatives.npz").stat().st_size


def test_the_grids_hold_the_edges():
    """A few of the edges the grids exist for, by name (a grid edited by hand must not lose them)."""
    f32 = np.float32
    x = C.unary_case("exp", f32)["x"]
    assert {87.0, -87.0, 16.0, -16.0} <= set(x) and x.max() > 88.72 and np.sum(x < -87.4) >= 10
    for op in ("sin", "cos", "tan"):
        x = C.unary_case(op, f32)["x"]
        assert {105615.0, float(np.nextafter(f32(105615.0), f32(np.inf)))} <= set(x) and np.abs(x).max() >= 1e30
    g = C.unary_case("gamma", f32)["x"]
    for k in range(1, 6):
        assert float(np.nextafter(f32(-k), f32(0))) in g and float(np.nextafter(f32(-k), f32(-np.inf))) in g
    assert {0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 8388607.0, 8388609.0} <= set(C.unary_case("round", f32)["x"])
    for op in ("floor", "ceil", "sign", "relu", "abs", "neg"):
        x = C.unary_case(op, f32)["x"]
        assert np.any((x == 0) & np.signbit(x)) and np.any((x == 0) & ~np.signbit(x)), op
    assert 1.0 in C.unary_case("acosh", f32)["x"]
    div = np.concatenate([b["y"] for b in C.binary_blocks("/", f32)])
    for k in (-45, 45, -50):
        assert {float(np.nextafter(f32(2.0 ** k), f32(0))), 2.0 ** k, float(np.nextafter(f32(2.0 ** k), f32(np.inf)))} <= set(div)
    assert np.any((np.abs(div) < 1.1754944e-38) & (div != 0))  # subnormal divisors
    m = C.binary_blocks("mod", f32)
    assert {(np.sign(a), np.sign(b)) for a, b in zip(m[0]["x"], m[0]["y"])} >= {(1, 1), (1, -1), (-1, 1), (-1, -1)}


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("op", C.unary_ops())
def test_oracle_unary_value(op, T):
    c = C.unary_case(op, T)
    got = C.oracle_unary(op, c["x"], T)
    pin = float(C.fixture()[f"una/{op}/{C.tname(T)}/oracle_err_ulp"])
    if C.is_exact(op):
        assert pin == 0.0
        same = C.same_bits(got, c["rn"])
        assert same.all(), (op, c["x"][~same][:4], got[~same][:4], c["rn"][~same][:4])
        return
    err = C.generator().ulp_err(got, c["hi"], c["lo"], T)
    w = int(np.argmax(err))
    print(f"{op} {np.dtype(T).name}: worst {err[w]:.4g} ulp at x = {c['x'][w]!r} (pinned {pin:.4g})")
    assert np.isfinite(got).all() and err[w] <= pin + 1e-6 and pin <= C.bar_ulp(op, T), (op, c["x"][w], got[w], c["hi"][w], err[w], pin)


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("op", C.binary_ops())
def test_oracle_binary_value(op, T):
    pin = float(C.fixture()[f"bin/{op}/{C.tname(T)}/oracle_err_ulp"])
    for k, c in enumerate(C.binary_blocks(op, T)):
        got = C.oracle_binary(op, c["x"], c["y"], T)
        if C.is_exact(op):
            same = C.same_bits(got, c["rn"])
            assert pin == 0.0 and same.all(), (op, k, c["x"][~same][:4], c["y"][~same][:4], got[~same][:4], c["rn"][~same][:4])
            continue
        err = C.generator().ulp_err(got, c["hi"], c["lo"], T)
        w = int(np.argmax(err))
        assert np.isfinite(got).all() and err[w] <= pin + 1e-6 and pin <= C.bar_ulp(op, T), (op, k, c["x"][w], c["y"][w], got[w], c["hi"][w])


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
def test_oracle_failures_and_conventions(T):
    """Every failure entry: not finite at the bad operand, finite at its neighbour. Every convention entry: the
    value written by hand, bit for bit."""
    fu, fb = C.fail_unary(T), C.fail_binary(T)
    assert {op for op, *_ in fu} >= {"log", "log2", "log10", "log1p", "sqrt", "acosh", "exp", "sinh", "cosh", "square", "cube",
                                       "gamma", "inv", "relu", "atanh_clip"}
    assert {op for op, *_ in fb} >= {"/", "pow", "mod", "+", "-", "*"}
    for op, bad, good, val in fu:
        b, g = C.oracle_unary(op, [bad, good], T)
        assert not np.isfinite(b) and np.isfinite(g), (op, bad, b, good, g)
        C.check_values(np.array([g]), op, T, C.point_case(op, T, val), f"{op} at {good!r}")
    for op, bx, by, gx, gy, val in fb:
        b, g = C.oracle_binary(op, [bx, gx], [by, gy], T)
        assert not np.isfinite(b) and np.isfinite(g), (op, bx, by, b, gx, gy, g)
        C.check_values(np.array([g]), op, T, C.point_case(op, T, val), f"{op} at ({gx!r}, {gy!r})")
    conv = C.conventions(T)
    assert len(conv) >= 70 and all(line for *_, line in conv)
    for op, x, y, want, line in conv:
        got = C.oracle_unary(op, [x], T)[0] if y is None else C.oracle_binary(op, [x], [y], T)[0]
        assert C.same_bits(got, T(want)), (op, x, y, got, want, line)


def test_cube_rounds_twice():
    """The stated deviation from RN_T(x^3): the reference computes x * x * x, and the fixture
    holds operands where that is one ulp from the correctly rounded cube."""
    from fractions import Fraction

    gen = C.generator()
    c = C.unary_case("cube", np.float32)
    direct = np.array([gen.rn(Fraction(float(v)) ** 3, np.float32) for v in c["x"]])
    assert np.any(direct != c["rn"].astype(np.float64))


def test_fixture_regenerates_bit_for_bit():
    """With mpmath at hand: a fixed subsample computed again equals the committed arrays bit for bit."""
    pytest.importorskip("mpmath")
    only = {"una/gamma", "una/cube", "una/erfc", "bin/pow", "bin/mod"}
    again = C.generator().generate(only=only)
    fx = C.fixture()
    assert len(again) > 40
    for k, v in again.items():
        a, b = np.asarray(v), np.asarray(fx[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k
