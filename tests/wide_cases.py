"""Shared by tests/test_wide_gpu.py: the trees, data and oracle results of the wide-dataset
tests (feature counts whose row tile does not fit in LDS), computed once per shape, shared
among the tests and never written to.

The inputs: random_population(ntrees, o, nfeat, T, seed=11) over {+, -, *, /, cos, exp},
X = default_rng(12).standard_normal((nfeat, n)), y = 2·cos(x_nfeat) + x_1² − 2, weights
|default_rng(13).standard_normal(n)|. Random trees rarely read the last feature, so every
batch ends with hand-made trees that do (hand_trees).
"""
import functools

import numpy as np

import oracle
import srhip
from numerics import loss_spread
from srhip import Node

OPS = (("+", "-", "*", "/"), ("cos", "exp"))
ARITH = (("+", "-", "*", "/"), ())


def deep_tree(o, nfeat, depth=6):
    """A balanced tree over + - * of `depth` levels, more than two stack slots, whose
    deepest leaf (one level below every other) is x_nfeat."""
    B = o.make_binary
    k = [0]

    def bal(d, leftmost):
        if d == 0:
            if leftmost:
                return B("*", Node(feature=nfeat), Node(feature=2))
            k[0] += 1
            return Node(feature=1 + (7 * k[0]) % nfeat)
        return B(("+", "-", "*")[d % 3], bal(d - 1, leftmost), bal(d - 1, False))

    return bal(depth, True)


def hand_trees(o, nfeat):
    """x_nfeat; the fused two-feature forms x_1·x_nfeat and x_nfeat/x_1; a deep tree reading
    x_nfeat at its deepest leaf; with cos / exp among the operators also cos(x_nfeat) + c and
    exp(exp(exp(x_nfeat·50))), which overflows and must fail."""
    B = o.make_binary
    last, first = (lambda: Node(feature=nfeat)), (lambda: Node(feature=1))
    trees = [last(), B("*", first(), last()), B("/", last(), first()), deep_tree(o, nfeat)]
    if "cos" in o.unary_operators:
        U = o.make_unary
        trees += [B("+", U("cos", last()), Node(val=0.75)),
                  U("exp", U("exp", U("exp", B("*", last(), Node(val=50.0)))))]
    return trees


@functools.lru_cache(maxsize=None)
def problem(T, nfeat, n=700, ntrees=200, ops=OPS, read=None, classes=False):
    """(options, trees, flat, X, y, w). `read`: the trees read features 1..read only (the
    dataset still has nfeat). `classes`: y ∈ {−1, +1}, the sign of the regression target."""
    T = np.dtype(T).type
    o = srhip.Options(binary_operators=list(ops[0]), unary_operators=list(ops[1]))
    nr = read or nfeat
    trees = list(srhip.random_population(ntrees, o, nr, T, seed=11)) + hand_trees(o, nr)
    flat = srhip.flatten(trees, o, dtype=T)
    X = np.random.default_rng(12).standard_normal((nfeat, n)).astype(T)
    y = (T(2) * np.cos(X[nfeat - 1]) + X[0] * X[0] - T(2)).astype(T)
    if classes:
        y = np.where(y >= 0, 1, -1).astype(T)
    w = np.abs(np.random.default_rng(13).standard_normal(n)).astype(T)
    for a in (X, y, w):
        a.setflags(write=False)
    return o, trees, flat, X, y, w


@functools.lru_cache(maxsize=None)
def reference(T, nfeat, n=700, ntrees=200, weighted=False, loss=None):
    """The oracle's (losses in T, did_succeed, conditioned spread of the loss) of problem(...)
    for `loss` (default L2)."""
    o, trees, flat, X, y, w = problem(T, nfeat, n, ntrees)
    loss = loss or o.elementwise_loss
    wv = w if weighted else None
    with np.errstate(all="ignore"):
        _, ref, rok = oracle.eval_loss_batch(flat, X, y, wv, loss.kind, loss.params, dtype=T)
        wsum = float(n) if wv is None else float(wv.astype(np.float64).sum())
        spread = loss_spread(trees, o, X, y, wv, T, loss=loss) / wsum
    for a in (ref, rok, spread):
        a.setflags(write=False)
    return ref, rok, spread


@functools.lru_cache(maxsize=None)
def predictions(T, nfeat, n=700, ntrees=200, ops=ARITH, classes=False):
    """The oracle's per-row predictions and did_succeed of problem(..., ops) (bit-exact by the
    project's bar for + - * / trees)."""
    o, trees, flat, X, y, w = problem(T, nfeat, n, ntrees, ops, None, classes)
    with np.errstate(all="ignore"):
        yhat, ok = oracle.eval_trees(flat, X, dtype=T)
    yhat.setflags(write=False)
    ok.setflags(write=False)
    return yhat, ok
