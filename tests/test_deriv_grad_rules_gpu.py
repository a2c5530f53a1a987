"""Every operator's second-order rule (device_ops.h uop_d2 / bop_d2, grad2_interp.h) in the
per-row mode (srhip_eval_mixed_tree_array) against the independent fixture
tests/golden/second_derivatives.npz (closed forms from mpmath; make_second_derivative_golden.py).

Trees: op(c0 + x1) with c0 = -0.0 (the operand is the grid value bit for bit; the inner sum has
value x, ∂/∂x = ∂/∂c = 1 and no mixed partial, so the tree's mixed partial is f''(x)), and the
binary trees of derivative_cases.py: op(c0 + x1, x2) gives fxx along x1 and fxy along x2,
op(x1, c0 + x2) gives fxy along x1 and fyy along x2. Shallow and deep (a feature-only pad adds
stack need and an exact zero), both dtypes, 293 rows: one full 256-row tile and a partial one.

Bound (nothing fitted to the engine's results), the form test_derivative_rules_gpu.py uses:
rule_err_ulp (the fixture's: the rule as written, in T, with correctly rounded transcendentals)
+ 4 ulp of T per transcendental value that enters the rule multiplicatively + 2 ulp per divide
(counts next to each rule in the generator), in ulps of T of the true value, plus 4 x the movement
of the true value under a 4-ulp move of the operands. Convention points are checked by class.
The first derivative the mode returns next to the mixed one is held to derivatives.npz with the
first-order bound. Every point is checked."""
import functools
from pathlib import Path

import numpy as np
import pytest

import derivative_cases as D
import srhip
from srhip import Node
from srhip.engine import DeviceDataset, Program

pytestmark = pytest.mark.gpu

NROWS = D.NROWS
TIDS = dict(ids=lambda T: np.dtype(T).name)
GOLDEN = Path(__file__).resolve().parent / "golden"


@functools.lru_cache(maxsize=None)
def fx2():
    with np.load(GOLDEN / "second_derivatives.npz") as z:
        fx = {k: z[k] for k in z.files}
    for v in fx.values():
        v.setflags(write=False)
    return fx


def unary_ops2():
    return sorted(k[4:-7] for k in fx2() if k.startswith("una/") and k.endswith("/ntrans"))


def binary_ops2():
    return sorted(k[4:-7] for k in fx2() if k.startswith("bin/") and k.endswith("/ntrans"))


def mixed(ctx, trees, X, dirs, T):
    """(∂ŷ/∂x [nt, ndir, n], ∂²ŷ/∂x∂c [nc, ndir, n]) as float64."""
    ds = DeviceDataset(ctx, X.astype(T), np.zeros(X.shape[1], dtype=T))
    prog = Program(ctx, srhip.flatten(trees, D.options(), dtype=T), T, interpreted=True)
    der, mix, ok = prog.eval_mixed_tree_array(ds, [d - 1 for d in dirs])
    assert ctx.last_kernel_name() == ("grad_kernel_deriv2_out<float>" if T == np.float32 else "grad_kernel_deriv2_out<double>")
    assert ok.all() and ctx.last_tree_code() == 0
    return der.astype(np.float64), mix.astype(np.float64), prog


def deepen(tree):
    """tree + (pad - pad): the pad's two copies cancel exactly (finite features), adding stack need and 0."""
    o = D.options()
    return o.make_binary("+", tree, o.make_binary("-", D.pad_tree(3), D.pad_tree(3)))


def check(got, true, spread, bound_ulp, T, what):
    err = D.ulp_err(got, true, T) * D.ulp_of(true, T)  # absolute; 0 where T rounds true to got's Inf
    tol = bound_ulp * D.ulp_of(true, T) + 4 * spread
    both_nan = np.isnan(got) & np.isnan(true)
    bad = ~both_nan & ~(err <= tol)
    worst = np.max(np.where(both_nan | (tol == 0), 0.0, err / np.where(tol > 0, tol, 1.0)))
    print(f"{what}: {len(got)} points, worst error / bound {worst:.3g}")
    assert not bad.any(), (what, np.flatnonzero(bad)[:5], got[bad][:5], true[bad][:5], tol[bad][:5])


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
@pytest.mark.parametrize("deep", [False, True], ids=["shallow", "deep"])
def test_unary_second_rules(gpu_ctx, T, deep):
    fx, tn = fx2(), D.tname(T)
    for op in unary_ops2():
        x = fx[f"una/{op}/{tn}/x"]
        X = np.zeros((3, NROWS))
        X[0] = D.rows_with_fill(x, op, T, 7)[:NROWS] if len(x) < NROWS else x[:NROWS]
        X[2] = 0.5
        tree = D.unary_tree(op)
        der, mix, prog = mixed(gpu_ctx, [deepen(tree) if deep else tree], X, [1], T)
        if deep:
            assert prog.pass_info()["grad_items"][3] >= 1
        n = len(x)
        bound = float(fx[f"una/{op}/{tn}/rule_err_ulp"]) + 4.0 * int(fx[f"una/{op}/ntrans"]) + 2.0 * int(fx[f"una/{op}/div"])
        check(mix[0, 0, :n], fx[f"una/{op}/{tn}/d2"], fx[f"una/{op}/{tn}/spread"], bound, T, f"{op} f'' {tn}")
        # the first derivative beside it: the first-order fixture on the points both grids hold
        x1, d1, s1 = D.unary_case(op, T)
        common = np.isin(x, x1)
        idx = np.searchsorted(x1, x[common])
        check(der[0, 0, :n][common], d1[idx], s1[idx], D.unary_bound_ulp(op, T), T, f"{op} f' {tn}")


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
@pytest.mark.parametrize("deep", [False, True], ids=["shallow", "deep"])
def test_binary_second_rules(gpu_ctx, T, deep):
    fx, tn, o = fx2(), D.tname(T), D.options()
    for op in binary_ops2():
        pre = f"bin/{op}/{tn}"
        x, y, bl = fx[f"{pre}/x"], fx[f"{pre}/y"], fx[f"{pre}/block"]
        bound = fx[f"{pre}/rule_err_ulp"] + 4.0 * fx[f"bin/{op}/ntrans"] + 2.0 * fx[f"bin/{op}/div"]
        for b in np.unique(bl):
            m = bl == b
            n = int(m.sum())
            X = np.ones((3, NROWS))
            X[0, :n], X[1, :n] = x[m], y[m]
            X[0, n:], X[1, n:] = x[m][0], y[m][0]
            trees = [o.make_binary(op, D.carrier(1), Node(feature=2)), o.make_binary(op, Node(feature=1), D.carrier(2))]
            if deep:
                trees = [deepen(t) for t in trees]
            der, mix, _ = mixed(gpu_ctx, trees, X, [1, 2], T)
            # where fxx is NaN by convention (pow at (0, 1): 0 · 0^-1) the first tree cannot show fxy alone: the
            # left operand's zero tangent along x2 still multiplies fxx (the first-order fixture's convention for a
            # leaf's zero tangent), so the reading there must be NaN; the second tree shows fxy itself
            nanxx = np.isnan(fx[f"{pre}/dxx"][m])
            for key, got, via_fxx in (("xx", mix[0, 0, :n], False), ("xy", mix[0, 1, :n], True), ("xy", mix[1, 0, :n], False),
                                      ("yy", mix[1, 1, :n], False)):
                k = ("xx", "xy", "yy").index(key)
                true = fx[f"{pre}/d{key}"][m]
                if via_fxx:
                    true = np.where(nanxx, np.nan, true)
                check(got, true, fx[f"{pre}/s{key}"][m], float(bound[k]), T, f"{op} f{key} {tn} block {b}")


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
def test_convention_points_by_class(gpu_ctx, T):
    fx, tn, o = fx2(), D.tname(T), D.options()
    for op, x, t, cls in zip(fx["conv/una/op"], fx["conv/una/x"], fx["conv/una/T"], fx["conv/una/cls"]):
        if t not in ("both", tn):
            continue
        X = np.full((2, NROWS), float(x))
        _, mix, _ = mixed(gpu_ctx, [D.unary_tree(str(op))], X, [1], T)
        assert all(D.class_matches(v, str(cls), T) for v in mix[0, 0, :4]), (op, x, cls, mix[0, 0, :4])
    for i, (op, x, y, t) in enumerate(zip(fx["conv/bin/op"], fx["conv/bin/x"], fx["conv/bin/y"], fx["conv/bin/T"])):
        if t not in ("both", tn):
            continue
        X = np.ones((2, NROWS))
        X[0], X[1] = float(x), float(y)
        trees = [o.make_binary(str(op), D.carrier(1), Node(feature=2)), o.make_binary(str(op), Node(feature=1), D.carrier(2))]
        _, mix, _ = mixed(gpu_ctx, trees, X, [1, 2], T)
        for key, got, via_fxx in (("xx", mix[0, 0, 0], False), ("xy", mix[0, 1, 0], True), ("xy", mix[1, 0, 0], False),
                                  ("yy", mix[1, 1, 0], False)):
            cls = str(fx[f"conv/bin/cls_{key}"][i])
            if via_fxx and str(fx["conv/bin/cls_xx"][i]) == "nan":
                cls = "nan"  # the first tree's zero tangent along x2 multiplies the NaN fxx (test_binary_second_rules)
            assert cls == "-" or D.class_matches(got, cls, T), (op, x, y, key, cls, got)
