"""Shared by tests/test_operator_values.py (CPU) and tests/test_operator_values_gpu.py:
the operator-value fixture (tests/golden/operators.npz, written by
tests/golden/make_operator_golden.py from exact rational arithmetic and mpmath), the
project's per-operator bars, and the comparison of a family's results with it.

Bounds (nothing fitted to what the engine returns):
  exact operators   (+ - * / neg abs square cube sqrt relu round floor ceil sign inv max min mod greater and
                    the logical operators) the bits of RN_T(true value), signed zero included;
  transcendentals   |got - true| <= 4 ulp_T(true); gamma 16 ulp;
  Float32 exp / sin / cos on the PRECISE paths: 0.5 ulp + 2^-28 |true| (test_precise_transcendentals.py);
  the FAST region's exp / sin / cos: 2 ulp, applied to the loss sums by
  test_operator_values_gpu.LossBatch.bound.
Operands are exact, so there is no conditioning term, and every point is checked.
"""
import functools
import importlib.util
from pathlib import Path

import numpy as np

import derivative_cases as D
import oracle
import srhip
from srhip import Node

GOLDEN = Path(__file__).resolve().parent / "golden"
NROWS = 549  # 512 + 37: one full tile of every family's row tile (128, 256 or 512) plus a partial one
DTYPES = D.DTYPES
TNAME = D.TNAME
BASIC_UNARY, BASIC_BINARY = D.BASIC_UNARY, D.BASIC_BINARY
PRECISE_F32 = ("exp", "sin", "cos")

ulp_of = D.ulp_of
options = D.options
tname = D.tname


@functools.lru_cache(maxsize=None)
def generator():
    """The generator module (numpy only at import; mpmath is imported by generate())."""
    spec = importlib.util.spec_from_file_location("make_operator_golden", GOLDEN / "make_operator_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN / "operators.npz") as z:
        fx = generator().unpack({k: z[k] for k in z.files})
    for v in fx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return fx


def unary_ops():
    return list(options().unary_operators)


def binary_ops():
    return list(options().binary_operators)


def is_exact(op):
    kind = "una" if op in unary_ops() else "bin"
    return bool(fixture()[f"{kind}/{op}/exact"])


def bar_ulp(op, T):
    """The bar for a transcendental operator in ulps of T (0 for an exact operator: the bits)."""
    kind = "una" if op in unary_ops() else "bin"
    return float(fixture()[f"{kind}/{op}/bar"])


def _true(fx, pre, T):
    """(hi, lo, rn or None) of a stored case: an exact operator stores rn alone."""
    if f"{pre}/rn" in fx:
        rn = fx[f"{pre}/rn"]
        return rn.astype(np.float64), np.zeros(len(rn)), rn
    hi = fx[f"{pre}/hi"]
    lo = fx[f"{pre}/lo_ulp"].astype(np.float64) * ulp_of(hi, np.float64) if np.dtype(T) == np.float64 else np.zeros(len(hi))
    return hi, lo, None


@functools.lru_cache(maxsize=None)
def unary_case(op, T):
    """dict(x [as float64], hi, lo, rn [in T, exact operators only])."""
    fx, pre = fixture(), f"una/{op}/{tname(T)}"
    hi, lo, rn = _true(fx, pre, T)
    return dict(x=fx[f"{pre}/x"].astype(np.float64), hi=hi, lo=lo, rn=rn)


@functools.lru_cache(maxsize=None)
def binary_blocks(op, T):
    """[dict(a, b, x, y, hi, lo, rn)]: block k is the product a x b, row-major (x repeats, y cycles)."""
    fx, pre = fixture(), f"bin/{op}/{tname(T)}"
    hi, lo, rn = _true(fx, pre, T)
    out, at = [], 0
    for k in range(int(fx[f"{pre}/nblocks"])):
        a, b = fx[f"{pre}/a{k}"].astype(np.float64), fx[f"{pre}/b{k}"].astype(np.float64)
        n = len(a) * len(b)
        out.append(dict(a=a, b=b, x=np.repeat(a, len(b)), y=np.tile(b, len(a)), hi=hi[at:at + n], lo=lo[at:at + n],
                        rn=None if rn is None else rn[at:at + n]))
        at += n
    assert at == len(hi)
    return out


def fail_unary(T):
    """[(op, bad operand, the nearest finite one, the value there)] for dtype T."""
    fx = fixture()
    return [(str(o), float(b), float(g), float(v)) for o, t, b, g, v in zip(fx["fail/una/op"], fx["fail/una/T"], fx["fail/una/bad"],
                                                                           fx["fail/una/good"], fx["fail/una/good_val"])
            if t == tname(T)]


def fail_binary(T):
    fx = fixture()
    return [(str(o), float(bx), float(by), float(gx), float(gy), float(v))
            for o, t, bx, by, gx, gy, v in zip(fx["fail/bin/op"], fx["fail/bin/T"], fx["fail/bin/bad_x"], fx["fail/bin/bad_y"],
                                               fx["fail/bin/good_x"], fx["fail/bin/good_y"], fx["fail/bin/good_val"]) if t == tname(T)]


def point_case(op, T, val):
    """A one-point case for check_values from a failure table's good_val."""
    v = np.array([val])
    return dict(x=v, hi=v, lo=np.zeros(1), rn=v.astype(T) if is_exact(op) else None)


def conventions(T):
    """[(op, x, y or None, expected value, the reference's line)] for dtype T."""
    fx = fixture()
    return [(str(o), float(x), None if np.isnan(y) else float(y), float(w), str(line))
            for o, x, y, t, w, line in zip(fx["conv/op"], fx["conv/x"], fx["conv/y"], fx["conv/T"], fx["conv/want"], fx["conv/line"])
            if t in ("both", tname(T))]


# ---- comparison ------------------------------------------------------------------------

def same_bits(got, want):
    """Equal as numbers of T and in the sign of a zero."""
    got, want = np.asarray(got), np.asarray(want)
    return (got == want) & (np.signbit(got) == np.signbit(want))


def bound(op, T, hi):
    """The absolute bound per point (0 for an exact operator)."""
    if is_exact(op):
        return np.zeros(len(hi))
    if np.dtype(T) == np.float32 and op in PRECISE_F32:
        return 0.5 * ulp_of(hi, T) + 2.0 ** -28 * np.abs(hi)
    return bar_ulp(op, T) * ulp_of(hi, T)


def value_ratio(got, op, T, case):
    """err / bound per point against a stored case (0 where an exact operator's bits agree, Inf where they do
    not or where the result is not finite)."""
    got = np.asarray(got)
    assert got.dtype == np.dtype(T) and got.shape == case["hi"].shape, (got.dtype, got.shape)
    if case["rn"] is not None:
        return np.where(same_bits(got, case["rn"]), 0.0, np.inf)
    with np.errstate(all="ignore"):
        err = np.abs((got.astype(np.float64) - case["hi"]) - case["lo"])
        r = err / bound(op, T, case["hi"])
    return np.where(np.isfinite(got) & ~np.isnan(r), r, np.inf)


def check_values(got, op, T, case, what):
    """Every point within its bound; returns the worst err / bound."""
    r = value_ratio(got, op, T, case)
    w = int(np.argmax(r))
    if not r[w] <= 1.0:
        bad = np.flatnonzero(~(r <= 1.0))
        at = [(case["x"][i], case["y"][i]) if "y" in case else case["x"][i] for i in bad[:4]]
        want = case["rn"] if case["rn"] is not None else case["hi"]
        raise AssertionError(f"{what}: {len(bad)} of {len(r)} points beyond the bound; at {at}: got {np.asarray(got)[bad[:4]]!r}, "
                             f"true {want[bad[:4]]!r}, err/bound {r[bad[:4]]}")
    return float(r[w])


# ---- the oracle, operator by operator ----------------------------------------------------

def opid(op):
    return generator().opid(op)


def oracle_unary(op, x, T):
    return generator().oracle_unary(op, x, T)


def oracle_binary(op, x, y, T):
    return generator().oracle_binary(op, x, y, T)


# ---- rows and trees ------------------------------------------------------------------------

def cycled(a, n=NROWS, start=0):
    """n rows cycling through a in its order (from index `start`), and each row's index in a."""
    idx = (np.arange(n) + start) % len(a)
    return np.asarray(a)[idx], idx


def feat(f):
    return Node(feature=f)


def U(op, child):
    return options().make_unary(op, child)


def B(op, l, r):
    return options().make_binary(op, l, r)


def zero_pad(feature, depth=6):
    """A balanced feature-only subtree of 2^depth leaves whose value is exactly +0.0 for every finite x: each
    pair of leaves is x - x = +0.0, and the upper levels add and subtract +0.0 (+0.0 ± +0.0 = +0.0 in round to
    nearest). Stack need depth - 1 >= 5, as derivative_cases.pad_tree."""
    level = [B("-", feat(feature), feat(feature)) for _ in range(2 ** (depth - 1))]
    k = 0
    while len(level) > 1:
        level = [B("+" if (k + i) % 2 else "-", level[i], level[i + 1]) for i in range(0, len(level), 2)]
        k += 1
    return level[0]
