"""Shared by tests/test_expr_ops.py and tests/test_expr_ops_gpu.py: the expression operators
of the feature, the options that hold them, and the expansion that the checker runs on.

The oracle has no custom operators. The checker is therefore the oracle on the EXPANDED tree:
`expand` substitutes every expression-operator node by its body, with x1 / x2 of the body
replaced by (copies of) the node's expanded arguments.

Two groups (srhip_internal.h uop_lossy / bop_lossy_*):
 - NONLOSSY: bodies built only from operators that propagate a non-finite operand (cos, sin,
   square, +, *). Every value inside such a body that is non-finite makes the body's result
   non-finite, so expansion cannot change did_succeed.
 - LOSSY: bodies with exp, inv or / inside. `nexp(x) = inv(exp(x))` where exp overflows gives 0
   and succeeds as an operator; its expansion fails at exp's output.

The definitions are the reference's (test/test_custom_operators.jl, test_derivatives.jl,
test_simplification.jl) written with engine operators: x^2 is square(x), 1/u is inv(u).
"""
import functools

import numpy as np

import srhip
from srhip import Node

# the primitives: the operators of the random trees plus everything a body uses
PRIM_BIN = ["+", "-", "*", "/"]
PRIM_UNA = ["cos", "exp", "sin", "square", "inv", "log"]


@functools.lru_cache(maxsize=None)
def prim_options():
    return srhip.Options(binary_operators=list(PRIM_BIN), unary_operators=list(PRIM_UNA))


def _xy():
    return Node("x1"), Node("x2")


def custom_cos(o):
    """custom_cos(x) = cos(x)^2"""
    x, _ = _xy()
    return o.make_unary("square", o.make_unary("cos", x))


def op3(o):
    """op3(x) = sin(x) + cos(x)"""
    return o.make_binary("+", o.make_unary("sin", Node("x1")), o.make_unary("cos", Node("x1")))


def my_func_a(o):
    """my_func_a(x, y) = x^2 * y"""
    x, y = _xy()
    return o.make_binary("*", o.make_unary("square", x), y)


def my_func_c(o):
    """my_func_c(x, y) = x*y + 0.3: a body constant"""
    x, y = _xy()
    return o.make_binary("+", o.make_binary("*", x, y), Node(val=0.3))


def nexp(o):
    """nexp(x) = inv(exp(x))"""
    return o.make_unary("inv", o.make_unary("exp", Node("x1")))


def op2(o):
    """op2(x, y) = x^2 + 1/(y^2 + 0.1)"""
    x, y = _xy()
    return o.make_binary("+", o.make_unary("square", x),
                         o.make_unary("inv", o.make_binary("+", o.make_unary("square", y), Node(val=0.1))))


def dbl(o):
    """dbl(x) = x*x + x: the argument is used three times"""
    return o.make_binary("+", o.make_binary("*", Node("x1"), Node("x1")), Node("x1"))


def ulog(o):
    """ulog(x) = log(x): safe_log, NaN on a negative argument"""
    return o.make_unary("log", Node("x1"))


DEFS = {"custom_cos": (custom_cos, 1), "op3": (op3, 1), "my_func_a": (my_func_a, 2), "my_func_c": (my_func_c, 2),
        "nexp": (nexp, 1), "op2": (op2, 2), "dbl": (dbl, 1), "ulog": (ulog, 1)}
NONLOSSY = ("custom_cos", "op3", "my_func_a", "my_func_c")
LOSSY = ("nexp", "op2", "dbl")


@functools.lru_cache(maxsize=None)
def expr_op(name):
    """The registered ExprOp of a definition (one handle per process)."""
    o = prim_options()
    fn, arity = DEFS[name]
    return srhip.ExprOp(name, fn(o), o, arity)


@functools.lru_cache(maxsize=None)
def options(names, binary=("+", "-", "*", "/"), unary=("cos", "exp")):
    """Options whose operator lists are the primitives `binary` / `unary` followed by the
    expression operators `names` (a tuple), each in the list of its arity."""
    ops = [expr_op(n) for n in names]
    return srhip.Options(binary_operators=list(binary) + [p for p in ops if p.arity == 2],
                         unary_operators=list(unary) + [p for p in ops if p.arity == 1])


def expand(tree, o):
    """`tree` (built under `o`) with every expression operator replaced by its body, as a tree
    under prim_options(). Arguments used several times by a body are copied per use."""
    po = prim_options()
    xo = o.expr_operators

    def subst(body, args):  # body is built under prim_options()
        if body.degree == 0:
            return Node(val=body.val) if body.constant else args[body.feature - 1].copy()
        if body.degree == 1:
            return Node(body.op, subst(body.l, args))
        return Node(body.op, subst(body.l, args), subst(body.r, args))

    def ex(t):
        if t.degree == 0:
            return t.copy()
        if t.degree == 1:
            name = o.unary_operators[t.op - 1]
            if name in xo:
                return subst(xo[name].tree, [ex(t.l)])
            return po.make_unary(name, ex(t.l))
        name = o.binary_operators[t.op - 1]
        if name in xo:
            return subst(xo[name].tree, [ex(t.l), ex(t.r)])
        return po.make_binary(name, ex(t.l), ex(t.r))

    return ex(tree)


def const_map(tree, o):
    """For every constant leaf of expand(tree, o), in get_constants order: the index of the
    constant of `tree` it is a copy of, or -1 for a body constant."""
    xo = o.expr_operators
    counter = [0]

    def number(t):  # tree constants in leaf order (post-order = left to right)
        if t.degree == 0:
            if t.constant:
                counter[0] += 1
                return ("c", counter[0] - 1)
            return ("x", t.feature)
        if t.degree == 1:
            return (1, t.op, number(t.l))
        return (2, t.op, number(t.l), number(t.r))

    def leaves(m):
        if m[0] == "c":
            return [m[1]]
        if m[0] == "x":
            return []
        if m[0] == 1:
            name, kids = o.unary_operators[m[1] - 1], [leaves(m[2])]
        else:
            name, kids = o.binary_operators[m[1] - 1], [leaves(m[2]), leaves(m[3])]
        if name not in xo:
            return [i for k in kids for i in k]

        def body(b):
            if b.degree == 0:
                return [-1] if b.constant else list(kids[b.feature - 1])
            if b.degree == 1:
                return body(b.l)
            return body(b.l) + body(b.r)

        return body(xo[name].tree)

    return leaves(number(tree))


@functools.lru_cache(maxsize=None)
def problem(T, n, names=NONLOSSY, ntrees=250, tree_seed=7, nfeat=5, xscale=8.0):
    """Random trees over {+, -, *, /, cos, exp} plus the operators `names`, their expansions,
    and a dataset (computed once per shape, shared and never written to)."""
    T = np.dtype(T).type
    o = options(tuple(names))
    trees = list(srhip.random_population(ntrees, o, nfeat, T, seed=tree_seed, maxsize=20))
    flat = srhip.flatten(trees, o, dtype=T)
    xflat = srhip.flatten([expand(t, o) for t in trees], prim_options(), dtype=T)
    # wide features: exp overflows on some rows, so that a fair share of the trees fails
    X = (xscale * np.random.default_rng(12).standard_normal((nfeat, n))).astype(T)
    y = (2 * np.cos(X[3]) + X[0] * X[0] - 2).astype(T)
    w = np.abs(np.random.default_rng(13).standard_normal(n)).astype(T)
    for a in (X, y, w):
        a.setflags(write=False)
    return o, trees, flat, xflat, X, y, w
