"""Shared by tests/test_derivative_rules.py (CPU) and tests/test_derivative_rules_gpu.py:
the derivative fixture (tests/golden/derivatives.npz, written by
tests/golden/make_derivative_golden.py from mpmath), the bounds derived from it, and
the trees that carry one operator's partials to a constant's gradient.

Constants that only exist to carry a tangent are -0.0: x + (-0.0) == x bit for bit
(test_feature_gradients.test_seeding_is_value_preserving), so the operand is the grid
value exactly. A constant that multiplies is 1.0 (x · 1.0 == x bit for bit).
"""
import functools
import importlib.util
from pathlib import Path

import numpy as np

import oracle
import srhip
from srhip import Node

GOLDEN = Path(__file__).resolve().parent / "golden"
NROWS = 293  # one full tile of the largest gradient row group (256) plus a partial one
TNAME = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
DTYPES = [np.float32, np.float64]
BASIC_UNARY = ("neg", "square", "cube", "exp", "abs", "log", "sqrt", "sin", "cos")  # srhip_internal.h kBasicUops
BASIC_BINARY = ("+", "-", "*", "/")  # kBasicBops


@functools.lru_cache(maxsize=None)
def generator():
    """The generator module (numpy only at import; mpmath is imported by generate())."""
    spec = importlib.util.spec_from_file_location("make_derivative_golden", GOLDEN / "make_derivative_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN / "derivatives.npz") as z:
        fx = {k: z[k] for k in z.files}
    for v in fx.values():
        v.setflags(write=False)
    return fx


@functools.lru_cache(maxsize=None)
def options():
    return generator().all_options()


def tname(T):
    return TNAME[np.dtype(T)]


def unary_ops():
    """Operators with a grid (gamma, whose rule is not provided, is not among them)."""
    fx = fixture()
    ops = sorted(k[4:-7] for k in fx if k.startswith("una/") and k.endswith("/ntrans"))
    return [o for o in ops if o not in set(fx["conv/deviations"])]


def binary_ops():
    return sorted(k[4:-7] for k in fixture() if k.startswith("bin/") and k.endswith("/ntrans"))  # "/" is one of them


def zero_unary():
    return [str(s) for s in fixture()["zero/una"]]


def zero_binary():
    return [str(s) for s in fixture()["zero/bin"]]


def ulp_of(t, T):
    return generator().ulp_of(t, T)


def ulp_err(got, true, T):
    return generator().ulp_err(got, true, T)


def unary_case(op, T):
    fx, pre = fixture(), f"una/{op}/{tname(T)}"
    return fx[f"{pre}/x"], fx[f"{pre}/d"], fx[f"{pre}/spread"]


def unary_bound_ulp(op, T):
    """oracle_err_ulp + 4 ulp per transcendental value that enters the rule multiplicatively (the per-operator
    bar of numerics.py) + 2 ulp for the rule's own divide or v_rcp_f32 (counts: make_derivative_golden.py)."""
    fx = fixture()
    return float(fx[f"una/{op}/{tname(T)}/oracle_err_ulp"]) + 4.0 * int(fx[f"una/{op}/ntrans"]) + 2.0 * int(fx[f"una/{op}/div"])


def binary_case(op, T):
    fx, pre = fixture(), f"bin/{op}/{tname(T)}"
    return {k: fx[f"{pre}/{k}"] for k in ("x", "y", "block", "dx", "dy", "sx", "sy")}


def binary_bound_ulp(op, T):
    """(d/dx, d/dy) bounds in ulps of T, as unary_bound_ulp."""
    fx = fixture()
    return (fx[f"bin/{op}/{tname(T)}/oracle_err_ulp"] + 4.0 * fx[f"bin/{op}/ntrans"] + 2.0 * fx[f"bin/{op}/div"]).astype(float)


def classify(v):
    v = float(v)
    if np.isnan(v):
        return "nan"
    if np.isinf(v):
        return "+inf" if v > 0 else "-inf"
    return "0" if v == 0 else "val"


def class_matches(v, cls, T):
    """v is of the hand-written class: "0", "+inf", "-inf", "nan", or exactly the number written."""
    if cls in ("0", "+inf", "-inf", "nan"):
        return classify(v) == cls
    return float(v) == float(np.dtype(T).type(float(cls)))


def conv_unary(T):
    """[(op, x, class)] of the convention table for dtype T."""
    fx = fixture()
    return [(str(o), float(x), str(c)) for o, x, t, c in zip(fx["conv/una/op"], fx["conv/una/x"], fx["conv/una/T"], fx["conv/una/cls"])
            if t in ("both", tname(T))]


def conv_binary(T):
    fx = fixture()
    return [(str(o), float(x), float(y), str(cx), str(cy))
            for o, x, y, t, cx, cy in zip(fx["conv/bin/op"], fx["conv/bin/x"], fx["conv/bin/y"], fx["conv/bin/T"],
                                          fx["conv/bin/cls_dx"], fx["conv/bin/cls_dy"]) if t in ("both", tname(T))]


def fill_range(op):
    return tuple(fixture().get(f"fill/{op}", np.array([-3.0, 3.0])))


def rows_with_fill(grid, op, T, seed):
    """NROWS operands: the grid first, then in-domain random values (Float32-rounded)."""
    lo, hi = fill_range(op)
    fill = np.random.default_rng(seed).uniform(lo, hi, NROWS - len(grid)).astype(np.float32).astype(np.float64)
    return np.concatenate([grid, fill])


# ---- trees ---------------------------------------------------------------------------

def carrier(feature):
    """(c0 + x_feature), c0 = -0.0: the feature's value with a constant's tangent."""
    return options().make_binary("+", Node(val=-0.0), Node(feature=feature))


def unary_tree(op, feature=1):
    """op(c0 + x_feature): ∂ŷ/∂c0 = op'(x_feature)."""
    return options().make_unary(op, carrier(feature))


def pad_tree(feature, depth=6):
    """A balanced feature-only subtree of 2^depth leaves: stack need depth - 1 (compile.cpp compute_need: an
    operator over two subtrees of equal need takes one more), no constants."""
    o = options()
    level = [Node(feature=feature) for _ in range(2 ** depth)]
    k = 0
    while len(level) > 1:
        level = [o.make_binary("+" if (k + i) % 2 else "-", level[i], level[i + 1]) for i in range(0, len(level), 2)]
        k += 1
    return level[0]


def oracle_grad(tree, X, T):
    """(ŷ, ∂ŷ/∂c [nconst][n] as float64, ok) of one tree by the oracle in T."""
    flat = srhip.flatten([tree], options(), dtype=T)
    k, a, c = flat.tree(0)
    with np.errstate(all="ignore"):
        v, g, ok = oracle.eval_grad_consts(k, a, c.astype(T), np.asarray(X, dtype=T), len(c), dtype=T)
    return v, g.astype(np.float64), ok


def oracle_unary_d(op, x, T):
    """The oracle's du of one operator in T at operands x (as float64)."""
    v, g, ok = oracle_grad(unary_tree(op), np.asarray(x, dtype=np.float64)[None, :], T)
    return v, g[0], ok


def oracle_binary_d(op, x, y, T):
    """The oracle's db of one operator in T: each partial alone, through op(c0 + x1, x2) and op(x1, c0 + x2)
    (a leaf operand's zero tangent still multiplies the other partial: see the convention table)."""
    o = options()
    X = np.stack([np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)])
    v, gx, ok = oracle_grad(o.make_binary(op, carrier(1), Node(feature=2)), X, T)
    _, gy, ok2 = oracle_grad(o.make_binary(op, Node(feature=1), carrier(2)), X, T)
    return v, gx[0], gy[0], ok and ok2
