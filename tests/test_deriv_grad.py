"""Constant gradients under a derivative objective, the parts that need no GPU (DESIGN.md
§3.19): the C prototypes against their Python mirror, the Python refusals, and the two
fixtures' generators (closed forms against mpmath.diff of the first-order closed forms;
the stored selection of trees)."""
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

import srhip
from srhip import Node, _lib

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
HEADER = (ROOT / "include" / "srhip.h").read_text()
NEW = ("srhip_eval_loss_grad_deriv", "srhip_eval_loss_grad_deriv_batch_ctx", "srhip_eval_mixed_tree_array",
       "srhip_optimize_constants_deriv")
OPTS = dict(binary_operators=["+", "-", "*"], unary_operators=["cos"])


def load(name):
    spec = importlib.util.spec_from_file_location(name, GOLDEN / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_prototypes_match_the_mirror():
    L = _lib.lib()
    for name in NEW:
        m = re.search(rf"^int32_t {name}\((.*?)\);", HEADER, re.M | re.S)
        assert m, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
        assert len(params) == len(_lib.SIGNATURES[name]), (name, params)
        assert hasattr(L, name)
    doc = HEADER[HEADER.index("derivative objectives: constant gradients"):HEADER.index("int32_t srhip_eval_loss_grad_deriv(")]
    for word in ("wide variant", "row sets", "group datasets", "expression", "tree code", "2^24", "256 constant groups"):
        assert word in doc, word
    assert "it needs ∂²ŷ/∂c∂x or finite differences" not in HEADER


def data(n=16):
    rng = np.random.default_rng(0)
    X = rng.standard_normal((3, n))
    return X, X[0] ** 2, np.stack([2 * X[0], np.zeros(n)])


def test_python_refusals_name_the_limit():
    X, y, g = data()
    ds = srhip.DerivativeDataset(X, y, g, [1, 2])
    obj = srhip.DerivativeObjective([1.0, 1.0, 1.0])
    o = srhip.Options(loss_function=obj, **OPTS)
    tree = o.make_binary("*", Node(val=2.0), Node("x1"))
    with pytest.raises(ValueError, match="row_idx"):
        srhip.optimize_constants_deriv_batch(ds, [tree], o, row_idx=np.zeros((1, 4), dtype=np.int64))
    with pytest.raises(ValueError, match="targets"):
        srhip.optimize_constants_deriv_batch(ds, [tree], o, targets=[0])
    with pytest.raises(ValueError, match="evaluator_factory"):
        srhip.optimize_constants_deriv_batch(ds, [tree], o, evaluator_factory=lambda c: None)
    with pytest.raises(ValueError, match="not supported"):  # no objective: only the value could be fitted
        srhip.optimize_constants_deriv_batch(ds, [tree], srhip.Options(**OPTS))
    with pytest.raises(ValueError, match="distance loss"):  # margin and expression losses
        srhip.optimize_constants_deriv_batch(ds, [tree], srhip.Options(loss_function=obj, elementwise_loss=srhip.L2MarginLoss(), **OPTS))
    with pytest.raises(ValueError, match="coefficients"):
        srhip.optimize_constants_deriv_batch(ds, [tree], srhip.Options(loss_function=srhip.DerivativeObjective([1.0, 1.0]), **OPTS))
    with pytest.raises(ValueError, match="Optimization function"):
        srhip.optimize_constants_deriv_batch(ds, [tree], srhip.Options(loss_function=obj, optimizer_algorithm="Adam", **OPTS))
    with pytest.raises(ValueError, match="start noise"):
        srhip.optimize_constants_deriv_batch(ds, [tree], o, noise=np.zeros(5))
    with pytest.raises(ValueError, match="DerivativeDataset"):  # a GroupDataset, or any other dataset
        srhip.optimize_constants_deriv_batch(srhip.Dataset(X, y), [tree], o)
    # optimize_constants_batch itself fits one target: it names the call that takes the objective
    with pytest.raises(ValueError, match="optimize_constants_deriv_batch"):
        srhip.optimize_constants_batch(ds, [tree], o)
    with pytest.raises(ValueError, match="DerivativeObjective"):
        srhip.eval_deriv_loss_grad_batch([tree], ds, srhip.Options(**OPTS))
    with pytest.raises(ValueError, match="DerivativeDataset"):
        srhip.eval_deriv_loss_grad_batch([tree], srhip.Dataset(X, y), o)


def test_second_order_closed_forms_against_mpmath_diff():
    """f'' is the derivative of the first-order fixture's closed form, and fxx / fxy / fyy those of its
    partials, on a handful of interior points (mpmath.diff at 60 digits; 1e-25 relative)."""
    import mpmath as mp

    mp.mp.dps = 60
    G2 = load("make_second_derivative_golden")
    U1, B1 = G2.G1.unary_rules(mp), G2.G1.binary_rules(mp)
    pts = {"acosh": [1.5, 3.25], "log": [0.5, 3.0], "log2": [0.5, 3.0], "log10": [0.5, 3.0], "sqrt": [0.5, 3.0],
           "log1p": [-0.5, 2.0], "atanh_clip": [0.3, -0.6]}
    for op, (f2, *_rest) in G2.second_unary(mp).items():
        if op in ("abs", "relu"):
            continue
        for x in pts.get(op, [0.7, -1.3]):
            want = mp.diff(U1[op].d, mp.mpf(x))
            got = f2(mp.mpf(x))
            assert abs(got - want) <= mp.mpf(10) ** -25 * (1 + abs(want)), (op, x, got, want)
    for op, (fxx, fxy, fyy, *_rest) in G2.second_binary(mp).items():
        if op in ("mod", "max", "min") or op in G2.G1.ZERO_BINARY:
            continue
        for x, y in ((1.5, 2.5), (0.75, -1.25)):
            a, b = mp.mpf(x), mp.mpf(y)
            r = B1[op]
            for got, want in ((fxx(a, b), mp.diff(r.dx, (a, b), (1, 0))), (fxy(a, b), mp.diff(r.dx, (a, b), (0, 1))),
                              (fxy(a, b), mp.diff(r.dy, (a, b), (1, 0))), (fyy(a, b), mp.diff(r.dy, (a, b), (0, 1)))):
                assert abs(got - want) <= mp.mpf(10) ** -25 * (1 + abs(want)), (op, x, y, got, want)


def test_second_derivative_fixture_is_the_generators():
    """A subsample regenerated: the committed file is what the generator writes."""
    G2 = load("make_second_derivative_golden")
    with np.load(GOLDEN / "second_derivatives.npz") as z:
        fx = {k: z[k] for k in z.files}
    sub = G2.generate(only={"una/tanh", "una/inv", "bin//", "bin/pow"})
    assert sub
    for k, v in sub.items():
        assert np.array_equal(fx[k], v, equal_nan=True), k
    assert (GOLDEN / "second_derivatives.npz").stat().st_size < 790_000


def test_deriv_grad_fixture_selection():
    G = load("make_deriv_grad_golden")
    with np.load(GOLDEN / "deriv_grad_cases.npz") as z:
        fx = {k: z[k] for k in z.files}
    trees = G.trees()
    assert len(trees) == int(fx["ntrees"]) == G.NRANDOM + 4 and len(fx["picked"]) == G.NRANDOM == 24
    nc = [len(G.const_nodes(t)) for t in trees]
    assert np.array_equal(np.cumsum([0] + nc), fx["const_off"]) and min(nc) >= 1
    assert sum(c > G.GC for c in nc[:G.NRANDOM]) >= 6
    assert fx["X"].shape == (4, 293) and list(fx["dirs"]) == [1, 3]
    for k in ("v", "dc", "dx", "dxc"):
        assert np.isfinite(fx[k]).all() and np.abs(fx[k]).max() < 1e6, k
    assert fx["dxc"].shape == (sum(nc), 2, 293) and np.abs(fx["dxc"]).max() > 0
    # one tree's rows regenerated
    t = 3
    base, move = G.evaluate(trees[t], fx["X"])
    assert np.array_equal(base[0], fx["v"][t])
    assert np.array_equal(G.encode(move["f32"][0]), fx["f32/sv"][t])
    assert (G.decode(fx["f64/sv"][t]) >= move["f64"][0]).all()
    assert (GOLDEN / "deriv_grad_cases.npz").stat().st_size < 790_000
