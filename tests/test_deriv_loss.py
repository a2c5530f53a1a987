"""Derivative objectives, host side (no GPU): DerivativeDataset / DerivativeObjective
validation, the objective's per-tree definition on a CPU evaluator (the oracle)
against analytic derivatives, and the ctypes prototypes against the header."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle
import srhip
from backends import OracleBackend
from srhip import _lib
from test_abi import HEADER
from test_feature_gradients import OPTS, analytic, eq1, eq2, oracle_feature_grad


def data(T=np.float64, n=40, nfeat=3, ndir=2, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random((nfeat, n)).astype(T) * 5, rng.standard_normal(n).astype(T),
            rng.standard_normal((ndir, n)).astype(T))


# ---- validation ---------------------------------------------------------------------
def test_dataset_layout():
    X, y, g = data()
    w = np.linspace(0.5, 1.5, 40)
    ds = srhip.DerivativeDataset(X, y, g, [3, 1], weights=w)
    assert isinstance(ds, srhip.Dataset) and ds.directions == (3, 1) and ds.ndir == 2 and ds.T == np.float64
    m = ds.multi
    assert m.ntargets == 3 and m.X is ds.X
    assert np.array_equal(m.Y, np.concatenate([y[None], g]))
    assert m.weights.shape == (3, 40) and all(np.array_equal(m.weights[k], w) for k in range(3))  # shared
    assert np.array_equal(ds.weights, w) and ds.weighted
    assert np.array_equal(ds.target(2).y, g[1])
    W = np.stack([w, 2 * w, 3 * w])
    ds = srhip.DerivativeDataset(X, y, g, [3, 1], weights=W)
    assert np.array_equal(ds.multi.weights, W) and np.array_equal(ds.weights, w)
    assert srhip.DerivativeDataset(X, y, g, [3, 1]).multi.weights is None


@pytest.mark.parametrize("bad", [
    dict(directions=[0, 1]), dict(directions=[1, 4]), dict(directions=[2, 2]), dict(directions=[1]),
    dict(directions=[1.5, 2]), dict(directions=[]), dict(directions=3),
    dict(y=np.zeros(39)), dict(y=np.zeros((1, 40))), dict(dydx=np.zeros((2, 39))), dict(dydx=np.zeros(40)),
    dict(X=np.zeros(40)), dict(y=np.zeros(40, dtype=np.float32)), dict(dydx=np.zeros((2, 40), dtype=np.float32)),
    dict(X=np.zeros((3, 40), dtype=np.int64)),
    dict(weights=np.ones(39)), dict(weights=np.ones((2, 40))), dict(weights=np.ones(40, dtype=np.float32)),
])
def test_dataset_validation_errors(bad):
    X, y, g = data()
    kw = dict(X=X, y=y, dydx=g, directions=[1, 2], weights=None)
    kw.update(bad)
    with pytest.raises(ValueError):
        srhip.DerivativeDataset(kw["X"], kw["y"], kw["dydx"], kw["directions"], kw["weights"])


def test_too_many_directions():
    X = np.zeros((20, 8))
    with pytest.raises(ValueError, match="1 to 15"):
        srhip.DerivativeDataset(X, np.zeros(8), np.zeros((16, 8)), list(range(1, 17)))


def test_objective_validation_errors():
    X, y, g = data()
    ds = srhip.DerivativeDataset(X, y, g, [1, 2])
    o = srhip.Options(**OPTS)
    for coef in ([1.0], [], [[1.0, 2.0]], [1.0, np.nan, 1.0], [1.0, np.inf]):
        with pytest.raises(ValueError):
            srhip.DerivativeObjective(coef)
    with pytest.raises(ValueError, match="distance loss"):
        srhip.DerivativeObjective([1, 1, 1], srhip.L1HingeLoss())
    with pytest.raises(ValueError, match="coefficients"):
        srhip.DerivativeObjective([1.0, 1.0])(eq1(o), ds, o)  # 2 coefficients, 3 channels
    with pytest.raises(ValueError, match="DerivativeDataset"):
        srhip.DerivativeObjective([1.0, 1.0, 1.0])(eq1(o), srhip.Dataset(X, y), o)
    with pytest.raises(ValueError, match="distance loss"):
        srhip.DerivativeObjective([1.0, 1.0, 1.0])(eq1(o), ds, srhip.Options(elementwise_loss=srhip.L2MarginLoss(), **OPTS))
    with pytest.raises(ValueError, match="DerivativeDataset"):
        srhip.eval_deriv_loss_batch([eq1(o)], srhip.Dataset(X, y), o)
    with pytest.raises(ValueError, match="not supported"):
        srhip.optimize_constants_batch(ds, [eq1(o)], o)
    obj = srhip.DerivativeObjective([1.0, 1.0, 1.0])
    oo = srhip.Options(loss_function=obj, **OPTS)
    with pytest.raises(ValueError, match="row_idx"):
        srhip.eval_loss_batch_ok([eq1(o)], ds, oo, row_idx=np.arange(4))


# ---- the per-tree definition on a CPU evaluator --------------------------------------
def cpu_objective(coef, loss=None):
    """The objective with the oracle behind its two evaluators."""
    ob = OracleBackend()

    def diff(tree, X, options, direction):
        v, G, ok = oracle_feature_grad(tree, options, np.asarray(X, dtype=np.float64), direction)
        return v, G[direction - 1], ok

    return srhip.DerivativeObjective(coef, loss, eval_tree_array=ob.eval_tree_array, eval_diff_tree_array=diff)


def host_rows(loss, r):
    ar = np.abs(r)
    if loss is None:
        return r * r
    if loss.kind == srhip.constants.LOSS["L1"]:
        return ar
    d = loss.param  # Huber
    return np.where(ar <= d, 0.5 * r * r, d * (ar - 0.5 * d))


@pytest.mark.parametrize("weights", [None, "shared", "channels"])
@pytest.mark.parametrize("loss", [None, srhip.L1DistLoss(), srhip.HuberLoss(1.0)])
def test_objective_against_analytic_derivatives(weights, loss):
    """eq1 and eq2 of test_feature_gradients.py: Σ_k coef_k · mean_k of the loss on ŷ and on
    the analytic ∂ŷ/∂x along each direction."""
    o = srhip.Options(**OPTS)
    rng = np.random.default_rng(0)
    X = rng.random((3, 100)) * 5
    dirs = [3, 1, 2]
    y = rng.standard_normal(100)
    g = rng.standard_normal((3, 100))
    W = {None: None, "shared": rng.uniform(0.5, 1.5, 100), "channels": rng.uniform(0.5, 1.5, (4, 100))}[weights]
    ds = srhip.DerivativeDataset(X, y, g, dirs, W)
    coef = np.asarray([1.0, 0.5, 2.0, 0.25])
    obj = cpu_objective(coef, loss)
    for j, eq in ((1, eq1), (2, eq2)):
        tree = eq(o)
        v, ok = OracleBackend().eval_tree_array(tree, X, o)
        assert ok
        A = analytic(j, X)
        chans = [(v, y)] + [(A[d - 1], g[k]) for k, d in enumerate(dirs)]
        Wk = np.ones((4, 100)) if W is None else np.broadcast_to(W, (4, 100))
        want = sum(c * np.sum(Wk[k] * host_rows(loss, p - t)) / np.sum(Wk[k]) for k, (c, (p, t)) in enumerate(zip(coef, chans)))
        got = obj(tree, ds, o)
        assert isinstance(got, np.float64)
        np.testing.assert_allclose(got, want, rtol=1e-9)


def test_objective_is_inf_on_failure_or_non_finite_result():
    o = srhip.Options(binary_operators=["+", "/"], unary_operators=["safe_sqrt"])
    X = np.asarray([[0.0, 1.0, 2.0], [1.0, 1.0, 1.0]])
    ds = srhip.DerivativeDataset(X, np.ones(3), np.ones((1, 3)), [1])
    obj = cpu_objective([1.0, 1.0])
    assert obj(o.make_binary("/", srhip.Node("x2"), srhip.Node("x1")), ds, o) == np.inf  # the value fails
    got = obj(o.make_unary("safe_sqrt", srhip.Node("x1")), ds, o)  # finite value, infinite slope at 0
    assert got == np.inf and isinstance(got, np.float64)
    f32 = srhip.DerivativeDataset(X.astype(np.float32), np.ones(3, np.float32), np.ones((1, 3), np.float32), [1])
    assert isinstance(obj(o.make_binary("+", srhip.Node("x1"), srhip.Node("x2")), f32, o), np.float32)


def test_combine_rule():
    obj = srhip.DerivativeObjective([1.0, 0.5])
    means = np.asarray([[1.0, 2.0], [np.nan, np.nan], [1.0, np.inf], [3.0, 4.0]])
    out = obj.combine(means, np.asarray([True, False, True, True]), np.float32)
    assert out.dtype == np.float32 and np.array_equal(out, np.asarray([2.0, np.inf, np.inf, 5.0], dtype=np.float32))


# ---- prototypes against the header -----------------------------------------------------
CTYPE = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "double": C.c_double}


@pytest.mark.parametrize("name", ["srhip_eval_loss_deriv", "srhip_eval_loss_deriv_batch_ctx"])
def test_ctypes_prototypes_match_header(name):
    m = re.search(rf"^int32_t\s+{name}\((.*?)\);", HEADER, re.M | re.S)
    assert m, f"{name} is not declared in include/srhip.h"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(params), (params, sig)
    for p, a in zip(params, sig):
        if "*" in p:
            assert a is C.c_void_p or issubclass(a, C._Pointer), (p, a)
            if "srhip_trees" in p:
                assert a is C.POINTER(_lib.Trees)
        else:
            assert a is CTYPE[p.split()[-2] if len(p.split()) > 1 else p], (p, a)
    assert hasattr(_lib.lib(), name)


def test_header_documents_the_limits():
    doc = HEADER[HEADER.index("derivative objectives: fused losses"):HEADER.index("int32_t srhip_eval_loss_deriv(")]
    for word in ("row sets", "group datasets", "constant optimisation", "expression losses", "tree code", "unpinned"):
        assert word in doc, word
