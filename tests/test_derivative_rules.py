"""The oracle's derivative rules (oracle/sr_oracle_ops.h du / db) against the independent
fixture tests/golden/derivatives.npz (closed forms from the mathematics, mpmath at 60
digits; tests/golden/make_derivative_golden.py).

The engine's rules (device_ops.h uop_d / bop_d) are checked against the oracle's
everywhere else; the two tables restate each other, so this file is what keeps a rule
that is wrong in both from passing. Bounds: the oracle's worst error in ulps of T as
the generator measured it (a regression pin, to 1e-6 ulp of slack for the division
by the ulp), and the generator's cap of 16 ulp asserted on its own. The convention
table (kinks, ties, poles with a finite value, the piecewise-constant operators, and
gamma's missing rule) is checked exactly, class by class.
"""
import numpy as np
import pytest

import derivative_cases as D

CAP = 16.0  # make_derivative_golden.MAX_ORACLE_ULP, stated again on purpose
TIDS = dict(ids=lambda T: np.dtype(T).name)


def test_the_fixture_covers_every_operator():
    """29 unary and 11 binary operators: each has a grid, or is piecewise constant, or is the stated deviation."""
    from srhip import constants as K

    fx = D.fixture()
    una = set(D.unary_ops()) | set(D.zero_unary()) | {str(s) for s in fx["conv/deviations"]}
    assert {n.lower() for n in K.UOPS} == una
    assert len(D.binary_ops()) == len(K.BOPS) == 11 and set(D.zero_binary()) <= set(D.binary_ops())
    assert D.generator().MAX_ORACLE_ULP == CAP and D.generator().MAX_ROWS == D.NROWS
    assert [str(s) for s in fx["conv/deviations"]] == ["gamma"]


def test_every_grid_point_has_a_finite_bound():
    """The bound against the fixture is B·ulp + 4·spread: an infinite spread would check nothing. The only
    points allowed one are the two Float32 acosh operands 1 and 2 ulps above 1 (a 4-ulp move leaves the
    domain), written out here; pow's negative bases and base 0 in particular have finite bounds."""
    fx = D.fixture()
    allowed = {("acosh", "f32"): [1.0 + 2.0 ** -23, 1.0 + 2.0 ** -22]}
    assert D.generator().INFINITE_SPREAD == allowed
    seen = 0
    for T in D.DTYPES:
        for op in D.unary_ops():
            x, d, sp = D.unary_case(op, T)
            assert sorted(x[~np.isfinite(sp)]) == allowed.get((op, D.tname(T)), []), (op, T)
            assert np.isfinite(D.unary_bound_ulp(op, T))
            seen += len(x)
        for op in D.binary_ops():
            c = D.binary_case(op, T)
            assert np.isfinite(c["sx"]).all() and np.isfinite(c["sy"]).all(), (op, T)
            assert np.isfinite(D.binary_bound_ulp(op, T)).all()
            seen += len(c["x"])
    c = D.binary_case("pow", np.float32)
    negative = c["x"] < 0
    assert negative.sum() >= 30 and np.all(c["y"][negative] == np.round(c["y"][negative]))
    assert np.any(c["sx"][negative] > 0)  # and the base's own conditioning is there
    assert seen > 5000


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
@pytest.mark.parametrize("op", D.unary_ops())
def test_oracle_unary_rule(op, T):
    x, d, _ = D.unary_case(op, T)
    assert 20 <= len(x) <= D.NROWS
    v, g, ok = D.oracle_unary_d(op, x, T)
    assert ok and np.isfinite(v).all(), (op, x[~np.isfinite(v)])
    err = D.ulp_err(g, d, T)
    w = int(np.argmax(err))
    pin = float(D.fixture()[f"una/{op}/{D.tname(T)}/oracle_err_ulp"])
    print(f"{op} {np.dtype(T).name}: worst {err[w]:.4g} ulp at x = {x[w]!r} (pinned {pin:.4g})")
    assert err[w] <= CAP, (op, x[w], g[w], d[w], err[w])
    assert err[w] <= pin + 1e-6, (op, x[w], g[w], d[w], err[w], pin)


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
@pytest.mark.parametrize("op", D.binary_ops())
def test_oracle_binary_rule(op, T):
    c = D.binary_case(op, T)
    v, gx, gy, ok = D.oracle_binary_d(op, c["x"], c["y"], T)
    assert ok and np.isfinite(v).all()
    pin = D.fixture()[f"bin/{op}/{D.tname(T)}/oracle_err_ulp"]
    for k, (what, g, d) in enumerate((("d/dx", gx, c["dx"]), ("d/dy", gy, c["dy"]))):
        err = D.ulp_err(g, d, T)
        w = int(np.argmax(err))
        print(f"{op} {what} {np.dtype(T).name}: worst {err[w]:.4g} ulp at ({c['x'][w]!r}, {c['y'][w]!r}) (pinned {pin[k]:.4g})")
        assert err[w] <= CAP, (op, what, c["x"][w], c["y"][w], g[w], d[w])
        assert err[w] <= pin[k] + 1e-6, (op, what, c["x"][w], c["y"][w], g[w], d[w], err[w], pin[k])
        if op in D.zero_binary():
            assert not g.any(), (op, what)


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
def test_oracle_conventions(T):
    """Every entry of the convention table, exactly: the class written by hand, or the number."""
    table = D.conv_unary(T)
    assert {op for op, _, _ in table} >= {"abs", "relu", "sqrt", "acosh", "inv", "gamma"} | set(D.zero_unary())
    for op in sorted({op for op, _, _ in table}):
        rows = [(x, cls) for o, x, cls in table if o == op]
        v, g, ok = D.oracle_unary_d(op, np.array([x for x, _ in rows]), T)
        assert ok, (op, v)  # value finite at every convention point
        for (x, cls), gi in zip(rows, g):
            assert D.class_matches(gi, cls, T), (op, x, cls, gi)
    tb = D.conv_binary(T)
    assert {op for op, *_ in tb} >= {"max", "min", "pow"} | set(D.zero_binary())
    for op in sorted({op for op, *_ in tb}):
        rows = [r[1:] for r in tb if r[0] == op]
        v, gx, gy, ok = D.oracle_binary_d(op, np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), T)
        assert ok, (op, v)
        for (x, y, cx, cy), a, b in zip(rows, gx, gy):
            assert D.class_matches(a, cx, T), (op, x, y, "d/dx", cx, a)
            assert cy == "-" or D.class_matches(b, cy, T), (op, x, y, "d/dy", cy, b)


def test_fixture_regenerates_bit_for_bit():
    """With mpmath at hand: a fixed subsample of the fixture computed again equals the committed arrays
    bit for bit (the fixture is what its generator says, the oracle_err_ulp pins included)."""
    pytest.importorskip("mpmath")
    only = {"una/atanh_clip", "una/tan", "una/erf", "una/acosh", "una/cube", "bin/pow", "bin/mod", "bin//"}
    again = D.generator().generate(only=only)
    fx = D.fixture()
    assert len(again) > 60
    for k, v in again.items():
        a, b = np.asarray(v), fx[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k
