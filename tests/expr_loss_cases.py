"""Shared by tests/test_expr_loss.py and tests/test_expr_loss_gpu.py: the loss
expressions E1-E5 of the expression-loss feature, problem A, and the checker.

The checker is the oracle applied twice: oracle.eval_trees gives ŷ and
did_succeed of the candidate trees; oracle.eval_tree on the loss expression over
the rows (ŷ_t, y, w) gives the per-row loss values in T and whether all of them
are finite; they are summed in float64.
"""
import functools

import numpy as np

import oracle
import srhip
from srhip import Node

LOSS_OPS = dict(binary_operators=["+", "-", "*", "/", "^"], unary_operators=["abs", "square", "log1p", "tanh", "log"])
ARITH = ("+", "-", "*", "/")


@functools.lru_cache(maxsize=None)
def loss_options():
    return srhip.Options(**LOSS_OPS)


def _ptw():
    return Node("x1"), Node("x2"), Node("x3")  # prediction, target, weight


def e1(o):
    """abs(p - t) ^ 2.5"""
    p, t, _ = _ptw()
    return o.make_binary("^", o.make_unary("abs", o.make_binary("-", p, t)), Node(val=2.5))


def e2(o):
    """square(p - t) / (abs(t) + 1): exactly rounded operators only"""
    p, t, _ = _ptw()
    return o.make_binary("/", o.make_unary("square", o.make_binary("-", p, t)),
                         o.make_binary("+", o.make_unary("abs", Node("x2")), Node(val=1.0)))


def e3(o):
    """w · log1p(square(p - t))"""
    p, t, w = _ptw()
    return o.make_binary("*", w, o.make_unary("log1p", o.make_unary("square", o.make_binary("-", p, t))))


def e4(o):
    """(p - t) · tanh(p - t): the prediction is used twice"""
    p, t, _ = _ptw()
    return o.make_binary("*", o.make_binary("-", p, t), o.make_unary("tanh", o.make_binary("-", Node("x1"), Node("x2"))))


def e5(o):
    """square(log(p / t)): non-finite on most rows"""
    p, t, _ = _ptw()
    return o.make_unary("square", o.make_unary("log", o.make_binary("/", p, t)))


def sq(o):
    """square(p - t): the built-in L2"""
    p, t, _ = _ptw()
    return o.make_unary("square", o.make_binary("-", p, t))


def wsq(o):
    """w · square(p - t): the weighted built-in L2"""
    p, t, w = _ptw()
    return o.make_binary("*", w, o.make_unary("square", o.make_binary("-", p, t)))


def absr(o):
    """abs(p - t): the built-in L1"""
    p, t, _ = _ptw()
    return o.make_unary("abs", o.make_binary("-", p, t))


EXPRS = {"E1": e1, "E2": e2, "E3": e3, "E4": e4, "E5": e5, "SQ": sq, "WSQ": wsq, "ABS": absr}
USES_W = {"E3", "WSQ"}


@functools.lru_cache(maxsize=None)
def loss_stream(name):
    """(kind, arg, consts as float64) of the expression's postfix stream."""
    o = loss_options()
    flat = srhip.flatten([EXPRS[name](o)], o, dtype=np.float64)
    return flat.tree(0)


@functools.lru_cache(maxsize=None)
def expr_loss(name):
    """The registered ExprLoss of an expression (one handle per process)."""
    o = loss_options()
    return srhip.ExprLoss(EXPRS[name](o), o)


def loss_rows(name, yhat, y, w, T):
    """The oracle's per-row loss values in T of one tree's predictions, and whether all are finite."""
    k, a, c = loss_stream(name)
    wcol = np.zeros_like(y) if w is None else w
    with np.errstate(all="ignore"):
        return oracle.eval_tree(k, a, c, np.stack([yhat, y, wcol]).astype(T), dtype=T)


def reference_sums(name, yhat, y, w, ok, T):
    """(Σ ℓ, Σ |ℓ|) per tree in float64 over the oracle's T-valued loss rows; NaN where the tree failed
    or a loss value is non-finite (the second array then holds NaN too)."""
    nt = yhat.shape[0]
    ref, mag = np.full(nt, np.nan), np.full(nt, np.nan)
    for t in np.flatnonzero(ok):
        rows, fin = loss_rows(name, yhat[t], y, w, T)
        if fin:
            r64 = rows.astype(np.float64)
            ref[t], mag[t] = r64.sum(), np.abs(r64).sum()
    return ref, mag


@functools.lru_cache(maxsize=None)
def problem(T, n, ntrees=200, tree_seed=11, extra_deep=False):
    """Problem A: `+ - * /` trees, a regression target, weights, and the oracle's per-row
    predictions (computed once per shape, shared and never written to). extra_deep appends
    the six trees of the deep family of tests/test_variant_matrix_gpu.py (balanced + - *
    trees needing 3 and 5 stack slots), which go to the deep interpreter variant."""
    T = np.dtype(T).type
    o = srhip.Options(binary_operators=list(ARITH), unary_operators=[])
    trees = list(srhip.random_population(ntrees, o, 5, T, seed=tree_seed))
    if extra_deep:
        from test_variant_matrix_gpu import family

        trees += [t.copy() for t in family("deep-eval")[0]]  # op indices 1..3 are + - * here too
    flat = srhip.flatten(trees, o, dtype=T)
    X = np.random.default_rng(12).standard_normal((5, n)).astype(T)
    y = (2 * np.cos(X[3]) + X[0] * X[0] - 2).astype(T)
    w = np.abs(np.random.default_rng(13).standard_normal(n)).astype(T)
    with np.errstate(all="ignore"):
        yhat, ok = oracle.eval_trees(flat, X, dtype=T)
    for a in (X, y, w, yhat, ok):
        a.setflags(write=False)
    return o, trees, flat, X, y, w, yhat, ok
