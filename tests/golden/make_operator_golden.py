"""Generate tests/golden/operators.npz — an independent reference for every
operator's VALUE (run by hand on the CPU:
python tests/golden/make_operator_golden.py; needs mpmath).

The derivative fixture (make_derivative_golden.py) pins the rules; this one pins
the values they rest on. Every kernel family carries its own copy of each operator
body, and the oracle restates device_ops.h line by line, so a convention that is
wrong in both passes every engine-against-oracle test. Here the expected value
comes from the mathematics: exact rational arithmetic (fractions.Fraction) for the
operators that are rational, mpmath at 80 digits for the others, at operands that
T holds exactly.

Per (operator, T in f32 / f64) three things are stored.

Value grids. `una/<op>/<T>/x` and the true value. An exact operator stores `rn`
alone: RN_T(true) in T, signed zero included (a zero's sign follows the IEEE / Julia
rule of the operator, ZERO_SIGN below); its bound is 0, so the bits decide. The
others store `hi` = RN_64(true) and, for Float64, `lo_ulp`: the rest true - hi in
ulps of Float64 at hi, as a Float32, so the reference's own error is negligible for
Float64 too (a Float32 result needs no rest: hi alone is within 2^-29 ulp of Float32).
All the small arrays are packed into one array per dtype (pack / unpack below).
Every grid value is finite in T (a failed tree's outputs are unspecified).
Grids start from the derivative generator's and add what matters for values (the
edges are named next to each grid). Binary operators are stored as blocks
`bin/<op>/<T>/a<k>`, `b<k>`: block k is the full product a<k> x b<k> in row-major
order, so a constant operand stays on the grid; `hi`, `lo_ulp` or `rn` hold the blocks one
after the other and `nblocks` their number.

Failure tables `fail/...`: operands (or pairs) whose value is not finite in T, with
the nearest operand where it still is. The class is written by hand; the "edge"
entries name a finite and a non-finite operand by hand and the generator bisects in
T with the mathematics (never the oracle) to the adjacent pair.

A convention table `conv/...`: points whose value mathematics does not fix (signed
zeros, ties, mod's sign, pow's special cases), the expected value written by hand
with the line of the reference package's source it follows.

Two operators are stated as the reference computes them, not as RN_T of the real
value:
  cube   x * x * x, two roundings (Operators.jl:35-36, Base.literal_pow): the stored
         value is the exact product RN_T(x * x) * x and rn its rounding;
  relu   (x + abs(x)) / 2 (Operators.jl:100-102): x + x overflows from floatmax / 2
         on, so those operands are failures.

The generator also evaluates the oracle in T at every point and stores its worst
error in ulps of T, `oracle_err_ulp`. It fails, naming the operator and the point,
when a point exceeds the operator's bar (0 for the exact operators, 4 ulp for the
transcendentals, 16 for gamma) or when a point's class disagrees with the oracle's.
"""
import io
import sys
import zipfile
from fractions import Fraction
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path[:0] = [str(ROOT / "symbolicregression.jl_amd"), str(ROOT / "oracle"), str(HERE)]
import make_derivative_golden as DG  # noqa: E402
from make_derivative_golden import F32_MIN, PI, above, around, geo, pm, r32, span  # noqa: E402

TYPES = DG.TYPES
MAX_POINTS = 256  # per grid or block
BAR_TRANS, BAR_GAMMA = 4.0, 16.0
F32_MAX = 3.4028234663852886e38
F64_MAX = 1.7976931348623157e308
F32_TINY = 1.401298464324817e-45  # smallest Float32 subnormal
F64_TINY = 5e-324
EXACT_UNARY = ("neg", "abs", "square", "cube", "sqrt", "relu", "round", "floor", "ceil", "sign", "inv")
EXACT_BINARY = ("+", "-", "*", "/", "max", "min", "mod", "greater", "logical_or", "logical_and")


# ---- exact rounding ---------------------------------------------------------------------

def F(x):
    return Fraction(float(x))


def mp_to_fraction(v):
    sign, man, exp, bc = v._mpf_
    # exp(-1e30) and the like: far below every subnormal / above every maximum; keep the rational short
    exp = max(min(int(exp), 5000 - bc), -5000 - bc) if man else 0
    f = Fraction(int(man)) * (Fraction(2) ** exp)
    return -f if sign else f


def rn(fr, T):
    """RN_T of an exact rational as a Float64 (±Inf past T's range); ties to even; the zero is +0."""
    fi = np.finfo(T)
    if fr == 0:
        return 0.0
    a = abs(fr)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, int(fi.minexp))
    q = Fraction(2) ** (e - int(fi.nmant))
    m = round(a / q)  # Fraction.__round__: ties to even
    v = m * q
    if v >= Fraction(2) ** (int(fi.maxexp)):
        out = np.inf
    else:
        out = float(v)  # exact: v is a number of T
    return -out if fr < 0 else out


def pair(fr):
    """(hi, lo) Float64 pair of an exact rational (hi ±Inf past Float64's range)."""
    hi = rn(fr, np.float64)
    if not np.isfinite(hi):
        return hi, 0.0
    return hi, rn(fr - Fraction(hi), np.float64)


# ---- the values -------------------------------------------------------------------------
# Exact operators take Fractions (and T) and return a Fraction; the others take and return mpmath numbers.

def fr_floor(q):
    return Fraction(q.numerator // q.denominator)


def fr_ceil(q):
    return -fr_floor(-q)


def fr_round_even(q):
    return Fraction(round(q))


def fr_mod(x, y):
    return x - y * fr_floor(x / y)


def unary_values(mp):
    def atanh_clip(x):
        u = fr_mod(mp_to_fraction(x) + 1, Fraction(2)) - 1  # exact, as x + 1 is on these grids
        return mp.atanh(mp.mpf(u.numerator) / mp.mpf(u.denominator))

    V = {
        "neg": lambda x, T: -x, "abs": lambda x, T: abs(x), "square": lambda x, T: x * x,
        "cube": lambda x, T: Fraction(rn(x * x, T)) * x,  # two roundings: see the module docstring
        "relu": lambda x, T: max(x, Fraction(0)), "round": lambda x, T: fr_round_even(x),
        "floor": lambda x, T: fr_floor(x), "ceil": lambda x, T: fr_ceil(x),
        "sign": lambda x, T: Fraction((x > 0) - (x < 0)), "inv": lambda x, T: 1 / x,
        "sqrt": mp.sqrt,  # irrational, but correctly rounded in T: 80 digits decide every rounding here
        "exp": mp.exp, "log": mp.log, "log2": lambda x: mp.log(x) / mp.log(2), "log10": mp.log10, "log1p": mp.log1p,
        "sin": mp.sin, "cos": mp.cos, "tan": mp.tan, "sinh": mp.sinh, "cosh": mp.cosh, "tanh": mp.tanh,
        "atan": mp.atan, "asinh": mp.asinh, "acosh": mp.acosh, "atanh_clip": atanh_clip, "erf": mp.erf, "erfc": mp.erfc,
        "gamma": mp.gamma,
    }
    return V


def binary_values(mp):
    one, zero = Fraction(1), Fraction(0)
    return {
        "+": lambda x, y: x + y, "-": lambda x, y: x - y, "*": lambda x, y: x * y, "/": lambda x, y: x / y,
        "max": lambda x, y: max(x, y), "min": lambda x, y: min(x, y), "mod": fr_mod,
        "greater": lambda x, y: one if x > y else zero,
        "logical_or": lambda x, y: one if (x > 0 or y > 0) else zero,
        "logical_and": lambda x, y: one if (x > 0 and y > 0) else zero,
        # pow: mpmath numbers; an integer exponent by exact rational powers when the result is short
        "pow": lambda x, y: mp.power(x, y),
    }


def neg0(v):
    return bool(np.signbit(v))


# The sign of an exact operator's zero result when the true value is 0 (True: -0.0): IEEE 754 / Julia Base.
ZERO_SIGN_UNARY = {
    "neg": lambda x: not neg0(x), "abs": lambda x: False, "square": lambda x: False, "cube": neg0, "sqrt": neg0,
    "relu": lambda x: False,  # (x + |x|) / 2: -0.0 + 0.0 = +0.0, x + |x| = +0.0 for x < 0
    "round": neg0, "floor": neg0, "ceil": neg0, "sign": neg0, "inv": lambda x: False,
}
ZERO_SIGN_BINARY = {
    "+": lambda x, y: (neg0(x) and neg0(y)) if (x == 0 and y == 0) else False,
    "-": lambda x, y: (neg0(x) and not neg0(y)) if (x == 0 and y == 0) else False,
    "*": lambda x, y: neg0(x) != neg0(y), "/": lambda x, y: neg0(x) != neg0(y),
    "mod": lambda x, y: neg0(y),  # Base.mod: copysign(r, y) when r == 0
    "max": lambda x, y: neg0(x) and neg0(y), "min": lambda x, y: neg0(x) or neg0(y),  # -0.0 < +0.0
    "greater": lambda x, y: False, "logical_or": lambda x, y: False, "logical_and": lambda x, y: False,
}


def signed_rn(fr, T, zero_is_negative):
    """RN_T with the zero's sign: the true value's when it is not 0 (an underflow keeps it), else the rule's."""
    v = rn(fr, T)
    if v == 0:
        return -0.0 if (fr < 0 or (fr == 0 and zero_is_negative)) else 0.0
    return v


# ---- the unary grids --------------------------------------------------------------------
# (extra Float32-rounded operands, extra Float64-only operands) on top of the derivative generator's grid.

def nb(c, ks):
    """Float64 neighbours of c: c moved by k Float64 ulps."""
    out = []
    for k in ks:
        v = np.float64(c)
        for _ in range(abs(k)):
            v = np.nextafter(v, np.inf if k > 0 else -np.inf)
        out.append(float(v))
    return out


def unary_extras():
    E = {}
    signs = [0.0, -0.0, F32_TINY, -F32_TINY, 1e-40, -1e-40, F32_MIN, -F32_MIN, 1.0, -1.0, 2.5, -2.5, 3e38, -3e38, F32_MAX,
             -F32_MAX]
    signs64 = [F64_TINY, -F64_TINY, 1e-310, -1e-310, F64_MAX, -F64_MAX, 1e300, -1e300]
    E["neg"] = (signs, signs64)
    E["abs"] = (signs, signs64)
    E["sign"] = (signs + pm(geo(1e-30, 1e30, 7)), signs64)
    # relu: ±0, subnormals, and up to floatmax / 2 (x + x must stay finite; beyond is a failure, below)
    E["relu"] = ([0.0, -0.0, F32_TINY, -F32_TINY, F32_MIN, -F32_MIN, 1.0, -1.0, 1.7e38, -3e38, -F32_MAX],
                 [F64_TINY, -F64_TINY, 8.9e307, -F64_MAX])
    # square: both sides of overflow (sqrt(floatmax) = 1.8446743e19; the far side is a failure), subnormal
    # results (|x| = 1e-19.5 .. 1e-22.4) and results that underflow to 0
    E["square"] = (pm([1.8446742e19, 1.84e19, 1e-19, 3e-20, 1e-20, 1e-21, 1e-22, 3.8e-23, 3.7e-23, 2.6e-23, 1e-23, F32_TINY,
                       F32_MIN]) + [0.0, -0.0],
                   pm([1.34078079e154, 1e-154, 1.5e-154, 1e-160, 2.3e-162, 1e-162, F64_TINY]))
    E["cube"] = (pm([6.9e12, 6.98e12, 1e-13, 2.2e-13, 1e-14, 1e-15, 1.12e-15, 1e-16, F32_TINY, 1.0000001, 3.0000002, 0.3]) + [0.0, -0.0],
                 pm([5.6e102, 1e-103, 1e-105, 1e-108, 1e-110, F64_TINY]))
    # inv: both sides of overflow (1 / 2.94e-39: a subnormal operand whose reciprocal is still finite),
    # subnormal results (|x| > 8.5e37)
    E["inv"] = (pm([3e-39, 5e-39, 1e-38, F32_MIN, 1e38, 3e38, F32_MAX, 8.5e37, 3.0, 7.0, 0.1]),
                pm([5.6e-309, 1e-308, 1e308, F64_MAX, 4.5e307]))
    E["sqrt"] = ([0.0, -0.0, F32_TINY, 1e-45, 3e-45, 1e-42, F32_MAX, 2.0, 3.0, 0.5, 0.1], [F64_TINY, 1e-310, F64_MAX, 2.0 ** -1022])
    # round: the ties (to even), 2^23 ± 1 (from 2^23 on every Float32 is an integer), ±0
    E["round"] = (pm([0.5, 1.5, 2.5, 3.5, 0.3, 0.7, 0.49999997, 0.50000006, 8388607.0, 8388609.0, 8388607.5, 8388608.0, 4194304.5,
                      4194305.5, 1e10, F32_TINY, 1e-40, F32_MAX]) + [0.0, -0.0],
                  pm([4503599627370495.5, 4503599627370497.0, 4503599627370496.0, 2251799813685248.5, 0.49999999999999994,
                      F64_TINY, F64_MAX]))
    fc = pm([0.5, 1.0, 1.5, 2.0, 0.99999994, 1.0000001, F32_TINY, 1e-40, 1e10, 8388607.5, 8388609.0, 3e38, 7.3]) + [0.0, -0.0]
    fc64 = pm([0.9999999999999999, 1.0000000000000002, F64_TINY, 4503599627370495.5, F64_MAX])
    E["floor"] = (fc, fc64)  # -0.5 and 0.5: results -1 / +0; ceil: -0 / 1
    E["ceil"] = (fc, fc64)
    # exp: both sides of |x| = 87 and 16 (the FAST guards); the last operands before overflow (88.72284 / 709.78);
    # the subnormal-result range is on the derivative grid (-104 .. -87.4), here its ends
    E["exp"] = (pm(around(87.0, (-1, 0, 1))) + pm(around(16.0, (-1, 0, 1))) + [88.0, 88.7, 88.72, 88.7228, -87.3, -87.4, -103.0,
                                                                                 -103.9, -103.97, -104.0, -110.0, -1e3, -1e30, 1e-30,
                                                                                 -1e-30, -0.0, 1e-40, 0.5, -0.5, 1.0],
                [709.0, 709.78, 709.7827, -708.3, -708.5, -744.0, -745.1, -745.2, -750.0, -1e300, 1e-300, 1e-17])
    big = pm([1e3, 3e4, 1.1e5, 1e6, 1e8, 3e10, 1e15, 1e22, 1e30, 1e38, 3e38])
    trig = (sum((around(k * PI / 2, (-1, 0, 1)) for k in (-2, -1, 1, 2, 3, 4, 5, 6, 100, 1001, 100000)), []) + big
            + pm(around(105615.0, (-2, -1, 0, 1, 2))) + pm([1e-30, 1e-40, F32_TINY, 1e-5, 0.5]) + [0.0, -0.0])
    trig64 = pm([1e-310, 1e100, 1e300, 1.5707963267948966, 3.141592653589793, 1e22])
    E["sin"] = (trig, trig64)
    E["cos"] = (trig, trig64)
    E["tan"] = (trig, trig64)
    # sinh / cosh: up to overflow (89.4159 / 710.4758)
    hyp = pm([88.7, 89.0, 89.4, 89.41, 89.415, 1e-40, F32_TINY, 1e-20, 0.5, 20.0, 50.0]) + [0.0, -0.0]
    E["sinh"] = (hyp, pm([710.0, 710.4, 710.475, 1e-310, 1e-200]))
    E["cosh"] = (hyp, pm([710.0, 710.4, 710.475, 1e-310, 1e-200]))
    # tanh / erf: tiny arguments (the value is x, 2x/sqrt(pi)), and where the result first rounds to ±1
    # (tanh 9.01 / 19.06, erf 3.92 / 5.93), far beyond
    E["tanh"] = (pm(geo(1e-30, 1e-3, 7) + [1e-40, F32_TINY, F32_MIN] + span(1.5, 8.5, 15) + around(9.0109, (-4, -2, -1, 0, 1, 2, 4))
                    + [8.6, 8.8, 9.2, 10.0, 20.0, 88.0, 100.0, 1e10, 3e38]) + [0.0, -0.0],
                 pm([18.0, 18.7, 19.0, 19.06, 19.1, 20.0, 40.0, 710.0, 1e300, 1e-310, 1e-200]))
    E["erf"] = (pm([1e-40, F32_TINY, F32_MIN, 1e-38, 0.84375, 0.85, 1.25, 2.857, 3.8, 3.9, 3.9192, 3.92, 3.95, 4.0, 6.0, 1e10, 3e38])
                + pm(around(3.9192, (-2, -1, 1, 2))) + [0.0, -0.0],
                pm([5.8, 5.9, 5.93, 5.95, 6.0, 1e300, 1e-310, 1e-200]))
    # erfc: down to its subnormal results (9.2 .. 10.05 / 26.55 .. 27.2) and 0; the negative side saturates to 2
    E["erfc"] = (pm([1e-40, 1e-20, 0.84375, 1.25, 2.857]) + [9.0, 9.19, 9.2, 9.5, 9.9, 10.0, 10.05, 10.06, 10.1, 11.0, 28.0, 1e10, 3e38,
                                                            -3.8, -3.9, -4.0, -4.2, -6.0, -1e10, -3e38, 0.0, -0.0],
                 [26.0, 26.5, 26.55, 26.6, 27.0, 27.2, 27.3, 28.0, 1e5, -5.8, -5.9, -6.0, -1e300])
    # log family: subnormal operands and the neighbours of 1
    lg = [F32_TINY, 3e-45, 1e-40, 5e-39, F32_MAX, 3e38] + around(1.0, (-4, -3, 3, 4)) + [0.5, 2.0, 10.0, 100.0, 1024.0, 2.7182817]
    lg64 = [F64_TINY, 1e-310, 1e-308, F64_MAX] + nb(1.0, (-2, -1, 1, 2)) + [2.718281828459045]
    for name in ("log", "log2", "log10"):
        E[name] = (lg, lg64)
    # log1p: just above -1 (on the derivative grid), tiny arguments (the value is x)
    E["log1p"] = (pm([1e-40, F32_TINY, F32_MIN, 1e-20, 1e-10, 1e-8, 6e-8]) + [0.0, -0.0, 3e38, F32_MAX, -0.5, -0.9999, 1e-3],
                  nb(-1.0, (1, 2)) + pm([1e-310, 1e-300, 1e-17, 1e-16]) + [F64_MAX])
    E["acosh"] = ([1.0] + above(1.0, (3, 4, 8, 100)) + [1.5, 2.0, 1e19, 1e30, 3e38, F32_MAX], nb(1.0, (1, 2, 3)) + [1e300, F64_MAX])
    far = pm(geo(1e19, 1e38, 6) + [1e-40, F32_TINY, 3e38]) + [0.0, -0.0]
    E["asinh"] = (far, pm([1e300, 1e-310, 1e-200, F64_MAX]))
    E["atan"] = (far + pm([1.0, 0.4375, 0.6875, 1.1875, 2.4375]), pm([1e300, 1e-310, 1e-200, F64_MAX]))
    E["atanh_clip"] = ([0.0, -0.0] + pm([2.0 ** -10, 2.0 ** -20, 0.5, 2.0, 4.0, 6.0, 1 - 2.0 ** -20, 3 - 2.0 ** -20]), [])
    # gamma: both sides of each pole -1 .. -5, half-integers, tiny positive arguments (Γ(x) = 1/x), up to the
    # overflow of T (35.04 / 171.62), negative non-integers whose value is a subnormal or underflows
    poles = sum((around(-float(k), (-2, -1, 1, 2)) for k in range(1, 6)), [])
    E["gamma"] = (poles + [k + 0.5 for k in range(-6, 12)] + [1e-30, 1e-38, 3e-39, 1e-10, 1e-5, -1e-5, -1e-10, -1e-30, -0.001, 0.001, 1.0,
                                                             2.0, 3.0, 10.0, 33.0, 34.0, 34.5, 35.0, 35.03, -33.5, -34.5, -35.5, -36.5,
                                                             -38.5, -40.5, -50.5, -100.5],
                  [100.0, 170.0, 170.9999999999999, 171.0, 171.00000000000003, 171.6, 171.62, 171.624376956302, -170.5, -171.5, -175.5, -177.5, -180.5, -190.5, 1e-300, 1e-308, -1e-300]
                  + sum((nb(-float(k), (-1, 1)) for k in range(1, 6)), []))
    return E


def unary_grid(mp, name, tname):
    """The derivative generator's grid (its Float64 extras with it) plus the extras above, sorted as a set."""
    dr = DG.unary_rules(mp).get(name)
    base = list(dr.grid) if dr else []
    base64 = list(dr.f64_extra) if dr else []
    if name == "atanh_clip":  # the derivative grid alone is 260 points: every second one
        base = base[::2]
    ex, ex64 = unary_extras()[name]
    g = np.concatenate([r32(base), r32(ex)])
    if name == "atanh_clip":  # x + 1 must be exact in Float32: the wrapped operand is then the one atanh really sees
        g = g[(g + 1.0).astype(np.float32).astype(np.float64) == g + 1.0]
    if tname == "f64":
        g = np.concatenate([g, np.asarray(base64 + list(ex64), dtype=np.float64)])
    # np.unique merges ±0: keep both zeros where the extras name -0.0
    u = np.unique(g)
    if any(v == 0 and np.signbit(v) for v in g) and any(v == 0 and not np.signbit(v) for v in g):
        i = int(np.flatnonzero(u == 0)[0])
        u = np.concatenate([u[:i], [-0.0, 0.0], u[i + 1:]])
    elif any(v == 0 and np.signbit(v) for v in g):
        u[u == 0] = -0.0
    return u


# ---- the binary blocks ------------------------------------------------------------------
# name -> (blocks for both types (Float32-rounded), Float64-only blocks). Every pair of a block has a finite value.

def binary_blocks():
    M, m, t = F32_MAX, F32_MIN, F32_TINY
    Bk = {}
    zeros = [0.0, -0.0]
    small = zeros + [1.0, -1.0, t, -t, 1e-40, -1e-40, m, -m, 0.1, 16777216.0, 1e-30, 1.7e38, -1.7e38, 3.0000002]
    # + -: signed zeros, subnormal results (m - nextafter(m), t - t), |x| + |y| up to floatmax; the overflow edge:
    # floatmax + y rounds back to floatmax below half an ulp (1.014e31), and the last ulps below it
    add_edge = ([M, 3e38, 2e38], [0.0, -0.0, 1.0, 1e30, 1e31, -1e31, -1e38, -3e38, -M])
    sub_edge = (add_edge[0], [-v for v in add_edge[1]])
    sub_m = (around(m, (0, 1, 2, 3)) + [-v for v in around(m, (0, 1, 2))], around(m, (0, 1, 2)) + [t, -t, 0.0])
    Bk["+"] = ([(small, small), add_edge, ([-M, -3e38], [-v for v in add_edge[1]]), sub_m],
               [([F64_MAX, 1e308], [0.0, 1.0, 1e291, -1e308, -F64_MAX]), ([F64_TINY, -F64_TINY, 2.0 ** -1022, 0.0], [F64_TINY, -F64_TINY, -2.0 ** -1022, -0.0])])
    Bk["-"] = ([(small, small), sub_edge, ([-M, -3e38], add_edge[1]), sub_m],
               [([F64_MAX, 1e308], [0.0, 1.0, -1e291, 1e308, F64_MAX]), ([F64_TINY, -F64_TINY, 2.0 ** -1022, 0.0], [F64_TINY, -F64_TINY, 2.0 ** -1022, 0.0])])
    # *: signed zeros, subnormal results and results that underflow to ±0 (ties at t / 2 included), the overflow edge
    Bk["*"] = ([(zeros + [1.0, -1.0, 1.5, -2.5, 1e-20, -1e-20, 1e-30, 1e19, -1e19, t, m, 3.0000002, 0.1],
                 zeros + [1.0, -1.0, 0.5, -0.5, 0.25, 0.75, 1e-20, 1e-25, -1e-25, 1e19, 3e18, 1.0000001, 7.0, 1e-8, 0.99999994]),
                ([M, -M, 2e38, 1e38], [1.0, -1.0, 0.5, 0.99999994, 1e-38, t, 1e-45 * 3, 0.0, -0.0, 1.5e-39])],
               [([F64_MAX, 1e300, -1e300, F64_TINY, 1e-300, 2.0 ** -1022], [1.0, -1.0, 0.5, 1e-8, 1e-30, 0.75, -0.25, 0.0])])
    # /: operands inside and on both sides of [2^-45, 2^45] (the packed division's range) and of 2^-50 (the FAST
    # bodies' lower bound); subnormal divisors, dividends and quotients; 0 / x
    rng_edges = sum((around(2.0 ** k, (-1, 0, 1)) for k in (-45, 45, -50)), []) + [2.0 ** -46, 2.0 ** 46, 2.0 ** -51, 2.0 ** -60]
    Bk["/"] = ([(zeros + [1.0, -1.0, 3.0, -7.0, 0.1, 1e-40, m, 1e-30] + rng_edges, [1.0, -1.0, 3.0, -7.0, 0.1, 1e-20, 1e20, 1e30, 3e38]),
                ([0.0, 1.0, -3.0] + rng_edges, [3.0] + rng_edges),
                (zeros + [1e-40, t, -1e-42, m, 1e-30, 1e-10, -1e-7], [1e-40, -1e-40, t, 5e-39, m, -t]),
                ([1e30, -1e30, 3e38, M, -M], [1.0, 3.0, 1e20, 3e38, -M, 2.0 ** 45, 1e38, 2.0 ** 46, 1.0000001, 7.0]),
                ([1e-30, 1e-38, m, 1e-40, 1.0, -1.0, 3.0, t], [1e8, 1e10, 3e38, 1e15, -1e7, M, 2.0 ** 100, 3.0])],
               [([1e300, 1e-300, F64_TINY, 1.0, F64_MAX, 2.0 ** -1022, 0.0], [1e5, 1e308, 3.0, -1e10, F64_MAX, 2.0]), ([1.0, 1e-300, -1.5], [1e-300, 1e-308, 2.0 ** -1022])])
    # pow: the derivative generator's blocks (positive bases with fractional exponents, negative and zero bases with
    # integer exponents, exponents 0, 1, 0.5, -1), subnormal and near-overflow results
    dpos = ([0.5, 1.0, 1.5, 2.0, 10.0, 1e-3, 0.999, 37.5], [-2.0, -1.0, 0.0, -0.0, 0.5, 1.0, 2.0, 2.5, 3.0, -0.75, 7.0])
    dneg = ([-2.0, -0.5, -1.0, -3.0, -10.0], [0.0, -0.0, 1.0, 2.0, 3.0, -1.0, -2.0, 5.0, 31.0, 20.0, -21.0])
    dzero = ([0.0, -0.0], [1.0, 2.0, 3.0, 0.5, 0.0, -0.0, 1e-30, 1e30])
    Bk["pow"] = ([dpos, dneg, dzero,
                  ([2.0, 0.5, 1.5, 0.75], [127.0, -127.0, 100.5, -100.5, 0.5, 1.0, 0.0, -1.0, 30.25, 126.99999]),
                  ([10.0], [38.0, -38.0, -40.0, -44.0, -44.8, -46.0, 38.5, -37.9]), ([2.0], [-126.0, -130.0, -149.0, -150.0, -151.0, -200.0, 127.99999]),
                  ([-2.0, -0.5], [127.0, -127.0, 126.0, -126.0]), ([1e-30, 1e30, t, M, 1.0], [1.0, 0.5, -0.5, 0.0, 0.25, 1e-30]),
                  ([1.0], [1e30, -1e30, 1e6, -1e7, 3e38]), ([1.0000001, 0.99999994], [1e6, -1e7, 1e8, -1e8])],
                 [([2.0], [1023.0, -1022.0, -1074.0, -1075.0, -1080.0, 0.5, 1000.5]), ([10.0], [308.0, -308.0, -320.0, -323.0, -330.0, 308.25])])
    # mod: every sign combination; quotients that are exact integers (the result is a zero with the divisor's
    # sign); huge quotients (Base.mod is exact there: it rests on rem, not on x - y floor(x / y))
    Bk["mod"] = ([([5.5, -5.5, 7.25, -7.25, 0.75, -0.75, 100.5, -100.5, 1e6 + 0.5, 0.0, -0.0, 6.0, -6.0, 1e-40, -1e-40],
                   [2.0, -2.0, 3.0, -3.0, 0.5, -0.5, 1.25, -1.25, 1e10, -1e10, 0.1, -0.1]),
                  ([1e30, -1e30, 3e38, -M, 1e10 + 1024, 16777216.0, -16777215.0, 1e20], [3.0, -3.0, 7.0, 0.1, -1e-5, 1e-30, t, 2.0, 1e38]),
                  ([t, -t, 1e-40, m, 3 * t], [t, -t, 2 * t, m, 1.0, -1.0])],
                 [([1e300, -1e300, F64_MAX, 9007199254740993.0], [3.0, -7.0, 0.1, 1e-300, F64_TINY])])
    mm = zeros + [1.0, -1.0, t, -t, M, -M, 2.5, 1e-40, -1e-40, 0.99999994]
    Bk["max"] = ([(mm, mm)], [([F64_TINY, -F64_TINY, 0.0, -0.0, F64_MAX], [F64_TINY, -F64_TINY, 0.0, -0.0, -F64_MAX])])
    Bk["min"] = Bk["max"]
    lg = zeros + [1.0, -1.0, 0.5, -0.5, t, -t, 2.0, M, -M, 1e-40]
    for name in ("greater", "logical_or", "logical_and"):
        Bk[name] = ([(lg, lg)], [([F64_TINY, -F64_TINY, 0.0, -0.0], [F64_TINY, -F64_TINY, 0.0, -0.0, 1.0])])
    return Bk


def blocks_of(name, tname):
    both, only64 = binary_blocks()[name]
    out = [(r32(a), r32(b)) for a, b in both]
    if tname == "f64":
        out += [(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)) for a, b in only64]
    return out


# ---- failures: hand-written classes -----------------------------------------------------
# (operator, T or "both", bad operand, the nearest operand that is still finite, why). An "edge" entry
# (EDGE_UNARY) names a finite and a non-finite operand; the generator bisects in T to the adjacent pair.

FAIL_UNARY = [
    ("log", "f32", 0.0, F32_TINY, "log(0) = -Inf: safe_log returns NaN at x <= 0 (Operators.jl:50-53)"),
    ("log", "f64", 0.0, F64_TINY, "as above"), ("log", "both", -0.0, 1.0, "-0.0 <= 0"), ("log", "both", -1.0, 1.0, "x < 0"),
    ("log", "f32", -F32_TINY, F32_TINY, "a negative subnormal"),
    ("log2", "f32", 0.0, F32_TINY, "Operators.jl:54-57"), ("log2", "f64", 0.0, F64_TINY, ""), ("log2", "both", -2.0, 2.0, "x < 0"),
    ("log10", "f32", 0.0, F32_TINY, "Operators.jl:58-61"), ("log10", "f64", 0.0, F64_TINY, ""), ("log10", "both", -10.0, 10.0, "x < 0"),
    ("log1p", "f32", -1.0, -0.99999994, "log1p(-1) = -Inf: NaN at x <= -1 (Operators.jl:62-65)"),
    ("log1p", "f64", -1.0, -0.9999999999999999, ""), ("log1p", "both", -2.0, 2.0, "x < -1"),
    ("log1p", "f32", -1.0000001, -0.99999994, "one ulp below -1"),
    ("sqrt", "both", -1.0, 1.0, "Operators.jl:70-73"), ("sqrt", "f32", -F32_TINY, -0.0, "sqrt(-0.0) = -0.0 is finite; the smallest negative number is not"),
    ("sqrt", "f64", -F64_TINY, -0.0, ""),
    ("acosh", "f32", 0.99999994, 1.0, "Operators.jl:66-69: NaN below 1; acosh(1) = 0"), ("acosh", "f64", 0.9999999999999999, 1.0, ""),
    ("acosh", "both", 0.0, 1.0, ""), ("acosh", "both", -2.0, 2.0, ""),
    ("exp", "both", 1000.0, 1.0, "overflow"), ("sinh", "both", 1000.0, 1.0, ""), ("sinh", "both", -1000.0, -1.0, ""), ("cosh", "both", -1000.0, 1.0, ""),
    ("square", "f32", 1e20, 1e19, ""), ("square", "f32", -3e38, -1e19, ""), ("cube", "f32", 1e13, 1e12, ""), ("cube", "f32", -1e20, -1e12, "x * x overflows first"),
    ("gamma", "both", 0.0, 1.0, "Γ(0) = Inf -> NaN (Operators.jl:8-11)"), ("gamma", "both", -0.0, 1.0, "-Inf -> NaN"),
    ("gamma", "f32", -1.0, -0.99999994, "a pole"), ("gamma", "f32", -2.0, -2.0000002, ""), ("gamma", "f32", -3.0, -2.9999998, ""),
    ("gamma", "f32", -4.0, -4.0000005, ""), ("gamma", "f32", -5.0, -4.9999995, ""), ("gamma", "f32", -100.0, -100.5, ""),
    ("gamma", "f64", -1.0, -0.9999999999999999, ""), ("gamma", "f64", -2.0, -2.0000000000000004, ""), ("gamma", "f64", -3.0, -2.9999999999999996, ""),
    ("gamma", "f64", -4.0, -4.000000000000001, ""), ("gamma", "f64", -5.0, -4.999999999999999, ""),
    ("gamma", "f32", 36.0, 35.0, "overflow"), ("gamma", "f64", 172.0, 171.0, "overflow"),
    ("gamma", "f32", 1e-39, 1e-38, "Γ(x) = 1/x overflows"),
    ("inv", "both", 0.0, 1.0, "1/0 = Inf"), ("inv", "both", -0.0, -1.0, "-Inf"), ("inv", "f32", F32_TINY, F32_MIN, "the reciprocal of a subnormal overflows"),
    ("inv", "f32", -1e-40, -F32_MIN, ""), ("inv", "f64", F64_TINY, 2.0 ** -1022, ""),
    ("relu", "f32", 3e38, 1.7e38, "(x + abs(x)) / 2: x + x overflows (Operators.jl:100-102)"), ("relu", "f32", F32_MAX, 1.7e38, ""),
    ("relu", "f64", F64_MAX, 8.9e307, ""),
    ("atanh_clip", "both", 1.0, 0.5, "mod(2, 2) - 1 = -1: atanh(-1) = -Inf (Operators.jl:14)"), ("atanh_clip", "both", -1.0, -0.5, "mod(0, 2) - 1 = -1"),
    ("atanh_clip", "both", 3.0, 2.5, ""), ("atanh_clip", "both", -3.0, -2.5, ""), ("atanh_clip", "both", 5.0, 4.5, ""), ("atanh_clip", "both", 101.0, 100.5, ""),
]
# (operator, T, a finite operand, a non-finite operand): the overflow edges
EDGE_UNARY = [
    ("exp", "f32", 88.0, 89.0), ("exp", "f64", 709.0, 710.0), ("sinh", "f32", 89.0, 90.0), ("sinh", "f32", -89.0, -90.0), ("sinh", "f64", 710.0, 711.0),
    ("cosh", "f32", 89.0, 90.0), ("cosh", "f32", -89.0, -90.0), ("cosh", "f64", -710.0, -711.0),
    ("square", "f32", 1e19, 2e19), ("square", "f32", -1e19, -2e19), ("square", "f64", 1e154, 2e154),
    ("cube", "f32", 6.9e12, 7e12), ("cube", "f32", -6.9e12, -7e12), ("cube", "f64", 5.6e102, 5.7e102),
    ("gamma", "f32", 35.0, 35.1), ("gamma", "f64", 171.6, 171.7), ("gamma", "f32", 3e-39, 2.9e-39),
    ("inv", "f32", 3e-39, 2.9e-39), ("inv", "f32", -3e-39, -2.9e-39), ("inv", "f64", 5.6e-309, 5.5e-309),
    ("relu", "f32", 1.7e38, 1.8e38), ("relu", "f64", 8.9e307, 9e307),
]
# (operator, T, bad x, bad y, good x, good y, why)
FAIL_BINARY = [
    ("/", "both", 1.0, 0.0, 1.0, 1.0, "x/0 = Inf"), ("/", "both", 1.0, -0.0, 1.0, -1.0, ""), ("/", "both", -3.0, 0.0, -3.0, 1.0, ""),
    ("/", "both", 0.0, 0.0, 0.0, 1.0, "0/0 = NaN"), ("/", "both", -0.0, 0.0, -0.0, 1.0, ""),
    ("/", "f32", 1.0, F32_TINY, 1.0, F32_MIN, "a subnormal divisor: the quotient overflows"), ("/", "f32", F32_MAX, 0.5, F32_MAX, 1.0, ""),
    ("/", "f32", 1e30, 1e-30, 1e30, 1e-8, ""), ("/", "f64", 1.0, F64_TINY, 1.0, 2.0 ** -1022, ""), ("/", "f64", F64_MAX, 0.5, F64_MAX, 1.0, ""),
    ("pow", "both", -2.0, 0.5, -2.0, 1.0, "a negative base and a fractional exponent (Operators.jl:42)"),
    ("pow", "both", -2.0, -0.5, -2.0, -1.0, "Operators.jl:43"), ("pow", "both", -0.5, 2.5, -0.5, 2.0, ""), ("pow", "both", -8.0, 1.0 / 3, -8.0, 1.0, ""),
    ("pow", "both", 0.0, -1.0, 0.0, 1.0, "0^-1 (Operators.jl:40)"), ("pow", "both", -0.0, -1.0, -0.0, 1.0, ""), ("pow", "both", 0.0, -0.5, 0.0, 0.5, "Operators.jl:43: x <= 0"),
    ("pow", "both", -0.0, -2.0, 2.0, -2.0, ""),
    ("pow", "f32", 10.0, 39.0, 10.0, 38.0, "overflow"), ("pow", "f32", 2.0, 128.0, 2.0, 127.0, ""), ("pow", "f32", -2.0, 129.0, -2.0, 127.0, "-Inf"),
    ("pow", "f32", 0.5, -128.0, 0.5, -127.0, ""), ("pow", "f64", 2.0, 1024.0, 2.0, 1023.0, ""), ("pow", "f64", 10.0, 309.0, 10.0, 308.0, ""),
    ("mod", "both", 5.5, 0.0, 5.5, 2.0, "mod(x, 0) = NaN"), ("mod", "both", 5.5, -0.0, 5.5, -2.0, ""), ("mod", "both", 0.0, 0.0, 0.0, 1.0, ""),
    ("mod", "both", -7.25, 0.0, -7.25, 3.0, ""),
    ("+", "f32", F32_MAX, F32_MAX, F32_MAX, 0.0, "overflow"), ("+", "f32", F32_MAX, 2e31, F32_MAX, 1e31, "floatmax + y rounds to Inf from half an ulp (1.014e31) on"),
    ("+", "f32", -3e38, -1e38, -3e38, -1e37, ""), ("+", "f64", F64_MAX, 1e292, F64_MAX, 1e291, ""),
    ("-", "f32", F32_MAX, -F32_MAX, F32_MAX, 0.0, ""), ("-", "f32", -F32_MAX, 2e31, -F32_MAX, 1e31, ""), ("-", "f64", F64_MAX, -1e292, F64_MAX, -1e291, ""),
    ("*", "f32", F32_MAX, 1.0000001, F32_MAX, 1.0, ""), ("*", "f32", 1e20, 1e20, 1e19, 1e19, ""), ("*", "f32", -1e30, 1e30, -1e30, 1e8, "-Inf"),
    ("*", "f64", F64_MAX, 1.0000000000000002, F64_MAX, 1.0, ""), ("*", "f64", 1e200, 1e200, 1e150, 1e150, ""),
]

# ---- conventions: (operator, x, y or None, T or "both", expected value, the reference's line) ----
B17 = "Operators.jl:17-18 (implicitly defined: Julia's Base)"
CONVENTIONS = [
    ("neg", 0.0, None, "both", -0.0, "Operators.jl:90-92: -x"), ("neg", -0.0, None, "both", 0.0, "Operators.jl:90-92"),
    ("abs", -0.0, None, "both", 0.0, B17), ("sqrt", -0.0, None, "both", -0.0, "Operators.jl:70-73: -0.0 < 0 is false, sqrt(-0.0) = -0.0"),
    ("square", -0.0, None, "both", 0.0, "Operators.jl:32-34"), ("cube", -0.0, None, "both", -0.0, "Operators.jl:35-37"),
    ("relu", -0.0, None, "both", 0.0, "Operators.jl:100-102: (-0.0 + 0.0) / 2 = +0.0"), ("relu", -1.0, None, "both", 0.0, "Operators.jl:100-102: (-1 + 1) / 2 = +0.0"),
    ("relu", 0.0, None, "both", 0.0, "Operators.jl:100-102"),
    ("sign", 0.0, None, "both", 0.0, B17 + ": sign(±0) = ±0"), ("sign", -0.0, None, "both", -0.0, B17), ("sign", F32_TINY, None, "both", 1.0, B17),
    ("round", 0.5, None, "both", 0.0, B17 + ": RoundNearest, ties to even"), ("round", -0.5, None, "both", -0.0, B17), ("round", 1.5, None, "both", 2.0, B17),
    ("round", -1.5, None, "both", -2.0, B17), ("round", 2.5, None, "both", 2.0, B17), ("round", -2.5, None, "both", -2.0, B17),
    ("round", 0.3, None, "both", 0.0, B17), ("round", -0.3, None, "both", -0.0, B17), ("round", 8388609.0, None, "both", 8388609.0, B17),
    ("round", 8388607.5, None, "both", 8388608.0, B17), ("round", 4194304.5, None, "both", 4194304.0, B17), ("round", 4194305.5, None, "both", 4194306.0, B17),
    ("floor", 0.5, None, "both", 0.0, B17), ("floor", -0.5, None, "both", -1.0, B17), ("floor", -0.0, None, "both", -0.0, B17), ("floor", 0.0, None, "both", 0.0, B17),
    ("ceil", -0.5, None, "both", -0.0, B17), ("ceil", 0.5, None, "both", 1.0, B17), ("ceil", -0.0, None, "both", -0.0, B17), ("ceil", 0.0, None, "both", 0.0, B17),
    ("+", 1.0, -1.0, "both", 0.0, "Operators.jl:23-25"), ("+", -0.0, -0.0, "both", -0.0, "Operators.jl:23-25"), ("+", -0.0, 0.0, "both", 0.0, "Operators.jl:23-25"),
    ("-", 0.0, 0.0, "both", 0.0, "Operators.jl:26-28"), ("-", -0.0, 0.0, "both", -0.0, "Operators.jl:26-28"), ("-", -0.0, -0.0, "both", 0.0, "Operators.jl:26-28"),
    ("*", -1.0, 0.0, "both", -0.0, "Operators.jl:29-31"), ("*", -0.0, -0.0, "both", 0.0, "Operators.jl:29-31"), ("*", -1e-30, 1e-30, "f32", -0.0, "Operators.jl:29-31: underflow keeps the sign"),
    ("/", 0.0, -1.0, "both", -0.0, "Operators.jl:47-49"), ("/", -0.0, -3.0, "both", 0.0, "Operators.jl:47-49"),
    ("max", 0.0, -0.0, "both", 0.0, "Base.max: -0.0 < +0.0"), ("max", -0.0, 0.0, "both", 0.0, "Base.max"), ("max", -0.0, -0.0, "both", -0.0, "Base.max"),
    ("min", 0.0, -0.0, "both", -0.0, "Base.min"), ("min", -0.0, 0.0, "both", -0.0, "Base.min"), ("min", 0.0, 0.0, "both", 0.0, "Base.min"),
    ("mod", 5.5, 2.0, "both", 1.5, B17 + ": the result has the divisor's sign"), ("mod", -5.5, 2.0, "both", 0.5, B17), ("mod", 5.5, -2.0, "both", -0.5, B17),
    ("mod", -5.5, -2.0, "both", -1.5, B17), ("mod", 6.0, -2.0, "both", -0.0, B17 + ": copysign(0, y)"), ("mod", -6.0, 2.0, "both", 0.0, B17),
    ("mod", 0.0, -3.0, "both", -0.0, B17), ("mod", -0.0, 3.0, "both", 0.0, B17), ("mod", 2.0 ** 100, 3.0, "both", 1.0, B17 + ": exact for a huge quotient (2^100 = 1 mod 3)"),
    ("pow", 0.0, 0.0, "both", 1.0, "Operators.jl:38-46: x^0 = 1"), ("pow", -2.0, 0.0, "both", 1.0, "Operators.jl:38-46"), ("pow", -2.0, 2.0, "both", 4.0, "Operators.jl:39"),
    ("pow", -2.0, 3.0, "both", -8.0, "Operators.jl:39"), ("pow", -0.0, 3.0, "both", -0.0, "Operators.jl:45: (-0.0)^3 = -0.0"), ("pow", -0.0, 2.0, "both", 0.0, "Operators.jl:45"),
    ("pow", 0.0, 0.5, "both", 0.0, "Operators.jl:42: 0 < 0 is false"), ("pow", -0.0, 0.5, "both", 0.0, "Operators.jl:42"), ("pow", 1.0, 1e30, "both", 1.0, "Operators.jl:45"),
    ("pow", -2.0, -1.0, "both", -0.5, "Operators.jl:39"), ("pow", 4.0, 0.5, "both", 2.0, "Operators.jl:45"),
    ("greater", 1.0, 1.0, "both", 0.0, "Operators.jl:94-96: x > y, a tie is 0"), ("greater", 0.0, -0.0, "both", 0.0, "Operators.jl:94-96"), ("greater", -1.0, -2.0, "both", 1.0, "Operators.jl:94-96"),
    ("logical_or", 0.0, 0.0, "both", 0.0, "Operators.jl:104-106: x > 0 || y > 0"), ("logical_or", -1.0, F32_TINY, "both", 1.0, "Operators.jl:104-106"),
    ("logical_or", -1.0, -0.0, "both", 0.0, "Operators.jl:104-106"), ("logical_and", 1.0, 0.0, "both", 0.0, "Operators.jl:109-111: x > 0 && y > 0"),
    ("logical_and", 2.0, F32_TINY, "both", 1.0, "Operators.jl:109-111"), ("logical_and", -1.0, -1.0, "both", 0.0, "Operators.jl:109-111"),
    # cube rounds twice (x * x, then * x): at these operands the result is one ulp from RN_T(x^3)
    ("cube", 1.0000008, None, "f32", 1.0000025, "Operators.jl:35-36: x^3 is x * x * x"),
]


# ---- evaluation -------------------------------------------------------------------------

def opid(name):
    from srhip import constants as K
    return K.OP_NAMES[name][1]


def oracle_unary(name, x, T):
    import oracle
    with np.errstate(all="ignore"):
        return np.array([oracle.unop(opid(name), T(v), T) for v in x], dtype=T)


def oracle_binary(name, x, y, T):
    import oracle
    with np.errstate(all="ignore"):
        return np.array([oracle.binop(opid(name), T(a), T(b), T) for a, b in zip(x, y)], dtype=T)


def true_unary(mp, name, x, T):
    """The true value of op(x) as a Fraction, or None where it is not a finite real number."""
    fn = unary_values(mp)[name]
    try:
        if name in EXACT_UNARY and name != "sqrt":
            return fn(F(x), T)
        v = fn(mp.mpf(float(x)))
    except (ZeroDivisionError, ValueError, OverflowError):
        return None
    if getattr(v, "imag", 0) != 0 or not mp.isfinite(v):
        return None
    return mp_to_fraction(mp.mpf(v.real) if hasattr(v, "real") else v)


def true_binary(mp, name, x, y, T):
    fn = binary_values(mp)[name]
    try:
        if name != "pow":
            return fn(F(x), F(y))
        if x == 0:  # 0^y: 1 at y = 0, 0 at y > 0, no value at y < 0
            return Fraction(1) if y == 0 else Fraction(0) if y > 0 else None
        if y == int(y) and abs(y) <= 64:
            return F(x) ** int(y)
        if x < 0 and y != int(y):
            return None
        if x < 0:  # an integer exponent too large for exact powers
            v = mp.power(-mp.mpf(float(x)), mp.mpf(float(y)))
            return mp_to_fraction(v) * (-1 if int(y) % 2 else 1)
        v = fn(mp.mpf(float(x)), mp.mpf(float(y)))
    except (ZeroDivisionError, ValueError, OverflowError):
        return None
    if getattr(v, "imag", 0) != 0 or not mp.isfinite(v):
        return None
    return mp_to_fraction(v)


def finite_in(fr, T):
    return fr is not None and np.isfinite(rn(fr, T))


def true_finite_unary(mp, name, x, T):
    if name == "relu" and x > 0 and not np.isfinite(rn(2 * F(x), T)):  # x + abs(x) overflows: see the module docstring
        return False
    if name == "cube" and not np.isfinite(rn(F(x) * F(x), T)):
        return False
    if name == "gamma" and x == 0:
        return False
    return finite_in(true_unary(mp, name, x, T), T)


def with_margin(mp, name, x, T, finite):
    """Is op(x) finite in T (or not: finite=False) whatever an error of the operator's bar does to it? An exact
    operator has no error; a result within `bar` ulps of floatmax may overflow or not, so the verdict at such an
    operand is not the operator's to give and the edge entries step past it."""
    if name in EXACT_UNARY:
        return true_finite_unary(mp, name, x, T) == finite
    fr = true_unary(mp, name, x, T)
    if fr is None:
        return not finite
    bar = BAR_GAMMA if name == "gamma" else BAR_TRANS
    moved = fr * (1 + Fraction(int(bar if finite else -bar)) * Fraction(2) ** -int(np.finfo(T).nmant))
    return bool(np.isfinite(rn(moved, T))) == finite


def bisect_edge(mp, name, T, good, bad):
    """Numbers of T (good, bad): op(good) finite in T, op(bad) not, by the mathematics: adjacent for an exact
    operator, else the nearest ones whose verdict holds within the operator's bar (with_margin)."""
    good, bad = _bisect_edge(mp, name, T, good, bad)
    g, b = T(good), T(bad)
    away = g - b  # from bad towards good and beyond
    while not with_margin(mp, name, g, T, True):
        g = np.nextafter(g, T(np.copysign(np.inf, away)))
    while not with_margin(mp, name, b, T, False):
        b = np.nextafter(b, T(np.copysign(np.inf, -away)))
    return float(g), float(b)


def _bisect_edge(mp, name, T, good, bad):
    good, bad = T(good), T(bad)
    assert true_finite_unary(mp, name, good, T) and not true_finite_unary(mp, name, bad, T), (name, good, bad)
    while True:
        mid = T(np.float64(good) / 2 + np.float64(bad) / 2)
        if mid == good or mid == bad:
            nxt = np.nextafter(good, bad, dtype=T) if T == np.float32 else np.nextafter(good, bad)
            if nxt == bad:
                return float(good), float(bad)
            mid = nxt
        if true_finite_unary(mp, name, mid, T):
            good = mid
        else:
            bad = mid


def ulp_err(got, hi, lo, T):
    """|got - (hi + lo)| in ulps of T at the true value."""
    with np.errstate(all="ignore"):
        d = np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)
        return d / DG.ulp_of(hi, T)


def store(out, pre, exact, hi, lo, rnv, T):
    """An exact operator stores `rn` alone (its bound is 0: the bits decide). The others store `hi`, and for
    Float64 `lo_ulp` = lo in ulps of Float64 at hi, as Float32 (a Float32 result needs no lo: hi alone is within
    2^-29 ulp of Float32)."""
    if exact:
        out[f"{pre}/rn"] = rnv.astype(T)
        return
    out[f"{pre}/hi"] = hi
    if T == np.float64:
        out[f"{pre}/lo_ulp"] = (lo / DG.ulp_of(hi, np.float64)).astype(np.float32)


def generate(only=None):
    """The fixture as a dict of arrays (only: a set of "una/<op>" / "bin/<op>" names, for the subsample check)."""
    import mpmath as mp

    mp.mp.dps = 80
    out, failed = {}, []
    una = DG.all_options().unary_operators
    bina = DG.all_options().binary_operators
    for name in una:
        if only is not None and f"una/{name}" not in only:
            continue
        exact = name in EXACT_UNARY
        bar = 0.0 if exact else BAR_GAMMA if name == "gamma" else BAR_TRANS
        out[f"una/{name}/exact"] = np.int8(exact)
        out[f"una/{name}/bar"] = np.float64(bar)
        for tname, T in TYPES.items():
            x = unary_grid(mp, name, tname)
            assert len(x) <= MAX_POINTS, (name, tname, len(x))
            assert np.array_equal(x.astype(T).astype(np.float64), x), (name, tname)
            pre = f"una/{name}/{tname}"
            hi, lo, rnv = np.empty(len(x)), np.empty(len(x)), np.empty(len(x))
            for i, v in enumerate(x):
                fr = true_unary(mp, name, v, T)
                if not true_finite_unary(mp, name, v, T):
                    failed.append(f"{name} {tname}: the value at x = {v!r} is not finite in T")
                    hi[i] = lo[i] = rnv[i] = np.nan
                    continue
                hi[i], lo[i] = pair(fr)
                rnv[i] = signed_rn(fr, T, ZERO_SIGN_UNARY[name](v)) if exact else rn(fr, T)
            got = oracle_unary(name, x, T)
            if exact:
                same = (got.astype(np.float64) == rnv) & (np.signbit(got) == np.signbit(rnv))
                err = np.where(same, 0.0, np.inf)
            else:
                err = ulp_err(got, hi, lo, T)
                err = np.where(np.isfinite(got), err, np.inf)
            w = int(np.argmax(err))
            if not err[w] <= bar:
                failed.append(f"{name} {tname}: the oracle is {err[w]:.3g} ulp off at x = {x[w]!r}: got {got[w]!r}, true {hi[w]!r}")
            out[f"{pre}/x"] = x.astype(T)
            store(out, pre, exact, hi, lo, rnv, T)
            out[f"{pre}/oracle_err_ulp"] = np.float64(err[w])
    for name in bina:
        if only is not None and f"bin/{name}" not in only:
            continue
        exact = name in EXACT_BINARY
        bar = 0.0 if exact else BAR_TRANS
        out[f"bin/{name}/exact"] = np.int8(exact)
        out[f"bin/{name}/bar"] = np.float64(bar)
        for tname, T in TYPES.items():
            pre = f"bin/{name}/{tname}"
            blocks = blocks_of(name, tname)
            out[f"{pre}/nblocks"] = np.int32(len(blocks))
            his, los, rns, worst = [], [], [], 0.0
            for k, (A, Bv) in enumerate(blocks):
                assert len(A) * len(Bv) <= MAX_POINTS, (name, tname, k, len(A) * len(Bv))
                assert np.array_equal(A.astype(T).astype(np.float64), A) and np.array_equal(Bv.astype(T).astype(np.float64), Bv)
                out[f"{pre}/a{k}"], out[f"{pre}/b{k}"] = A.astype(T), Bv.astype(T)
                xs, ys = np.repeat(A, len(Bv)), np.tile(Bv, len(A))
                hi, lo, rnv = np.empty(len(xs)), np.empty(len(xs)), np.empty(len(xs))
                for i, (a, b) in enumerate(zip(xs, ys)):
                    fr = true_binary(mp, name, a, b, T)
                    if not finite_in(fr, T):
                        failed.append(f"{name} {tname} block {k}: the value at ({a!r}, {b!r}) is not finite in T")
                        hi[i] = lo[i] = rnv[i] = np.nan
                        continue
                    hi[i], lo[i] = pair(fr)
                    rnv[i] = signed_rn(fr, T, ZERO_SIGN_BINARY[name](a, b)) if exact else rn(fr, T)
                got = oracle_binary(name, xs, ys, T)
                if exact:
                    same = (got.astype(np.float64) == rnv) & (np.signbit(got) == np.signbit(rnv))
                    err = np.where(same, 0.0, np.inf)
                else:
                    err = np.where(np.isfinite(got), ulp_err(got, hi, lo, T), np.inf)
                w = int(np.argmax(err))
                if not err[w] <= bar:
                    failed.append(f"{name} {tname} block {k}: the oracle is {err[w]:.3g} ulp off at ({xs[w]!r}, {ys[w]!r}): "
                                  f"got {got[w]!r}, true {hi[w]!r}")
                worst = max(worst, float(err[w]))
                his.append(hi), los.append(lo), rns.append(rnv)
            store(out, pre, exact, np.concatenate(his), np.concatenate(los), np.concatenate(rns), T)
            out[f"{pre}/oracle_err_ulp"] = np.float64(worst)
    if only is None:
        tables(mp, out, failed)
    if failed:
        raise SystemExit("\n".join(failed))
    return out


def good_value(fr, exact, T, zero_is_negative):
    if fr is None:
        return np.nan  # reported by the class check
    return signed_rn(fr, T, zero_is_negative) if exact else rn(fr, np.float64)


def tables(mp, out, failed):
    """The failure and convention tables, each entry checked against the mathematics and the oracle."""
    fu = []  # (op, T, bad, good)
    for op, tn, bad, good, _ in FAIL_UNARY:
        for t in (("f32", "f64") if tn == "both" else (tn,)):
            fu.append((op, t, float(TYPES[t](bad)), float(TYPES[t](good))))
    for op, tn, good, bad in EDGE_UNARY:
        g, b = bisect_edge(mp, op, TYPES[tn], good, bad)
        fu.append((op, tn, b, g))
    for op, tn, bad, good in fu:
        T = TYPES[tn]
        if true_finite_unary(mp, op, T(bad), T) or not true_finite_unary(mp, op, T(good), T):
            failed.append(f"failure table: {op} {tn} ({bad!r}, {good!r}) is not (non-finite, finite) by the mathematics")
        ob, og = oracle_unary(op, [bad, good], T)
        if np.isfinite(ob) or not np.isfinite(og):
            failed.append(f"failure table: the oracle disagrees at {op} {tn} ({bad!r} -> {ob!r}, {good!r} -> {og!r})")
    out["fail/una/op"] = np.array([f[0] for f in fu], dtype="U16")
    out["fail/una/T"] = np.array([f[1] for f in fu], dtype="U8")
    out["fail/una/bad"] = np.array([f[2] for f in fu], dtype=np.float64)
    out["fail/una/good"] = np.array([f[3] for f in fu], dtype=np.float64)
    # the value at the finite neighbour: RN_T(true) for an exact operator, RN_64(true) for the others
    out["fail/una/good_val"] = np.array([good_value(true_unary(mp, f[0], TYPES[f[1]](f[3]), TYPES[f[1]]), f[0] in EXACT_UNARY, TYPES[f[1]],
                                                    ZERO_SIGN_UNARY[f[0]](f[3]) if f[0] in EXACT_UNARY else False) for f in fu])
    fb = []
    for op, tn, bx, by, gx, gy, _ in FAIL_BINARY:
        for t in (("f32", "f64") if tn == "both" else (tn,)):
            T = TYPES[t]
            fb.append((op, t, float(T(bx)), float(T(by)), float(T(gx)), float(T(gy))))
    for op, tn, bx, by, gx, gy in fb:
        T = TYPES[tn]
        if finite_in(true_binary(mp, op, bx, by, T) if by != 0 or op not in ("/", "mod") else None, T) or \
                not finite_in(true_binary(mp, op, gx, gy, T), T):
            failed.append(f"failure table: {op} {tn} ({bx!r}, {by!r}) / ({gx!r}, {gy!r}) is not (non-finite, finite) by the mathematics")
        ob, og = oracle_binary(op, [bx, gx], [by, gy], T)
        if np.isfinite(ob) or not np.isfinite(og):
            failed.append(f"failure table: the oracle disagrees at {op} {tn} ({bx!r}, {by!r}) -> {ob!r}, ({gx!r}, {gy!r}) -> {og!r}")
    out["fail/bin/op"] = np.array([f[0] for f in fb], dtype="U16")
    out["fail/bin/T"] = np.array([f[1] for f in fb], dtype="U8")
    for j, key in enumerate(("bad_x", "bad_y", "good_x", "good_y")):
        out[f"fail/bin/{key}"] = np.array([f[2 + j] for f in fb], dtype=np.float64)
    for op, x, y, tn, want, _ in CONVENTIONS:
        for t in (("f32", "f64") if tn == "both" else (tn,)):
            T = TYPES[t]
            got = oracle_unary(op, [x], T)[0] if y is None else oracle_binary(op, [x], [y], T)[0]
            if not (got == T(want) and np.signbit(got) == np.signbit(T(want))):
                failed.append(f"convention table: the oracle gives {got!r} for {op}({x!r}{'' if y is None else ', ' + repr(y)}) in {t}, "
                              f"written {want!r}")
    out["fail/bin/good_val"] = np.array([good_value(true_binary(mp, f[0], f[4], f[5], TYPES[f[1]]), f[0] in EXACT_BINARY, TYPES[f[1]],
                                                    ZERO_SIGN_BINARY[f[0]](f[4], f[5]) if f[0] in EXACT_BINARY else False) for f in fb])
    out["conv/op"] = np.array([c[0] for c in CONVENTIONS], dtype="U16")
    out["conv/x"] = np.array([c[1] for c in CONVENTIONS], dtype=np.float64)
    out["conv/y"] = np.array([np.nan if c[2] is None else c[2] for c in CONVENTIONS], dtype=np.float64)
    out["conv/T"] = np.array([c[3] for c in CONVENTIONS], dtype="U8")
    out["conv/want"] = np.array([c[4] for c in CONVENTIONS], dtype=np.float64)
    out["conv/line"] = np.array([c[5] for c in CONVENTIONS], dtype="U96")


def pack(d):
    """The many small arrays of generate() as one array per dtype (a zip member costs more than most of them
    hold): `pack/<dtype>/data` holds them one after the other in the order of `names`, `len` their lengths
    (-1: a scalar). Tables of strings stay as they are."""
    out = {}
    d = {k: np.asanyarray(v) for k, v in d.items()}
    for dt in sorted({v.dtype.name for v in d.values() if v.dtype.kind in "fi"}):
        keys = sorted(k for k, v in d.items() if v.dtype.name == dt)
        out[f"pack/{dt}/names"] = np.array(keys, dtype="U48")
        out[f"pack/{dt}/len"] = np.array([-1 if d[k].ndim == 0 else d[k].size for k in keys], dtype=np.int32)
        out[f"pack/{dt}/data"] = np.concatenate([d[k].ravel() for k in keys])
    out.update({k: v for k, v in d.items() if v.dtype.kind not in "fi"})
    return out


def unpack(z):
    """The inverse of pack (z: a dict of arrays)."""
    out = {k: v for k, v in z.items() if not k.startswith("pack/")}
    for key in z:
        if key.startswith("pack/") and key.endswith("/names"):
            pre = key[:-len("names")]
            data, at = z[pre + "data"], 0
            for name, n in zip(z[key], z[pre + "len"]):
                out[str(name)] = data[at] if n < 0 else data[at:at + n]
                at += max(int(n), 1) if n < 0 else int(n)
    return out


def main():
    flat = generate()
    out = pack(flat)
    back = unpack(out)
    assert set(back) == set(flat) and all(np.array_equal(back[k], flat[k], equal_nan=flat[k].dtype.kind == "f")
                                          and np.array_equal(np.signbit(back[k]), np.signbit(flat[k]))
                                          for k in flat if np.asanyarray(flat[k]).dtype.kind == "f")
    path = Path(__file__).with_name("operators.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:  # as np.savez_compressed, with a fixed date: byte for byte
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    npts = sum(v.size for k, v in flat.items() if k.endswith("/hi") or k.endswith("/rn"))
    print("wrote", len(flat), "arrays in", len(out), ",", npts, "points,", path.stat().st_size, "bytes")
    for k in sorted(flat):
        if k.endswith("oracle_err_ulp"):
            print(f"  {k:40s} {np.round(flat[k], 3)}")


if __name__ == "__main__":
    main()
