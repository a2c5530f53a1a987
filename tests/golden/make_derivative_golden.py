"""Generate tests/golden/derivatives.npz — an independent reference for every
operator's derivative rule (run by hand on the CPU:
python tests/golden/make_derivative_golden.py; needs mpmath).

The constant gradients rest on two tables of local partials (device_ops.h
uop_d / bop_d) that the oracle's du / db restate line by line, so a rule that
is wrong in both passes every engine-against-oracle test. This fixture is the
third party: for every differentiable operator an explicit operand grid,
written by hand next to the rule, and the closed-form derivative from the
mathematics (not from either table), evaluated by mpmath at 60 digits at the
exact operand and rounded once to Float64.

Grids are given in Float64 and rounded to Float32, so both dtypes see an
operand they hold exactly; a grid may add Float64-only points (`f64_extra`).
Every grid keeps the operator's VALUE finite in T (a non-finite value fails
the tree, which is not what is tested here); the derivative may under- or
overflow T, and is then expected as T rounds it (0 / a subnormal / ±Inf).

Per (operator, T) the generator also evaluates the oracle's rule in T
(oracle.eval_grad_consts on op(c0 + x1), c0 = -0.0, so the operand is the grid
value bit for bit) and stores its worst error in ulps of T, `oracle_err_ulp`.
Every point must stay within MAX_ORACLE_ULP or the generator fails naming the
operator and the point: where the rule itself is ill-conditioned in T and the
reference package computes it the same way, the grid is narrowed by hand below,
with the reason; nothing is dropped at test time.

Stored per unary operator `una/<op>/<T>/`: x, d, spread (the movement of d
under a 4-ulp-of-T move of the operand: the operand's own conditioning),
oracle_err_ulp; `una/<op>/ntrans`, `una/<op>/div`: the bound's terms (below).
Per binary operator `bin/<op>/<T>/`: x, y, dx, dy, sx, sy, oracle_err_ulp (2),
block (the index of the operand block a point belongs to: a block is a full
product A x B of valid operands, so a tree with a constant operand stays in
the grid at every row).
`conv/...`: the conventions, points where mathematics gives no answer (or the
project knowingly deviates) and the expected class is written out by hand.

Bound terms (tests/test_derivative_rules_gpu.py): the engine may differ from
the true derivative by oracle_err_ulp + 4 ulp of T per transcendental value
that enters the rule multiplicatively (`ntrans`, the project's per-operator
bar) + 2 ulp if the rule divides (`div`: an IEEE divide or v_rcp_f32 plus the
rounding of its argument), plus the operand's conditioning.
"""
import sys
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "symbolicregression.jl_amd"), str(ROOT / "oracle")]

MAX_ORACLE_ULP = 16.0
MAX_ROWS = 293  # a grid (a binary block) fills one test batch: one full 256-row gradient tile and a partial one
TYPES = {"f32": np.float32, "f64": np.float64}
PI = 3.14159265358979323846


# ---- grid helpers (everything ends up rounded to Float32) --------------------------

def r32(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def span(lo, hi, n):
    return list(np.linspace(lo, hi, n))


def geo(lo, hi, n):
    return list(np.geomspace(lo, hi, n))


def pm(a):
    return list(a) + [-v for v in a]


def around(c, ks=(-16, -2, -1, 0, 1, 2, 16)):
    """Float32 neighbours of c: the Float32 nearest c moved by k Float32 ulps."""
    out = []
    for k in ks:
        v = np.float32(c)
        for _ in range(abs(k)):
            v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
        out.append(float(v))
    return out


def above(c, ks=(1, 2, 16, 1024)):
    return around(c, ks)


F32_MIN = 1.1754943508222875e-38  # smallest normal Float32
ERF_TAIL = pm([k / 8 for k in range(37, 85, 2)])  # 4.625 .. 10.375 (see erf below)


# ---- the rules ----------------------------------------------------------------------
# The closed forms take and return mpmath numbers.

@dataclass
class Unary:
    d: Callable            # the closed-form derivative
    grid: list             # operands (rounded to Float32)
    f64_extra: list        # Float64-only operands, as they are
    ntrans: int            # transcendental values that enter the rule multiplicatively
    div: int               # 1 if the rule ends in a divide / reciprocal
    reason: str            # one line on ntrans / div


@dataclass
class Binary:
    dx: Callable           # the closed-form partials
    dy: Callable
    blocks: list           # [(A, B), ...]: each block is a full product of valid operands
    ntrans: tuple          # (for d/dx, for d/dy), as Unary.ntrans
    div: tuple
    moves_y: Callable = field(default=lambda x, y: True)  # whether the conditioning move touches y at (x, y)


def unary_rules(mp):
    one = mp.mpf(1)

    def u_of(x):  # the operand atanh sees in atanh_clip: mod(x + 1, 2) - 1 (floored mod)
        s = x + 1
        return s - 2 * mp.floor(s / 2) - 1

    trig = (span(-8, 8, 41)
            # next to multiples of pi/2 (small and large ones), where sin or cos is tiny
            + sum((around(k * PI / 2) for k in (-4, -3, -2, -1, 1, 2, 3, 4, 100, 1001)), [])
            # the fast reduction ends at |x| = 105615 (device_ops.h trig_big): both sides, and far beyond
            + pm(around(105615.0, (-1, 0, 1))) + pm([1e3, 3e4, 1.1e5, 1e6, 1e8, 3e10, 1e15, 1e22, 1e30]))
    R = {}
    R["neg"] = Unary(lambda x: -one, pm(geo(1e-30, 1e30, 13)) + [0.0], [], 0, 0, "constant")
    R["square"] = Unary(lambda x: 2 * x, pm(geo(1e-18, 1e18, 25)) + [0.0, 1e-40, -1e-40], [1e150, -1e-150], 0, 0,
                   "2x is exact (a subnormal x included)")
    # 3x^2 at |x| = 1e-20 .. 1e-22 is a Float32 subnormal (the value x^3 underflows to 0: finite)
    R["cube"] = Unary(lambda x: 3 * x * x, pm(geo(1e-12, 1e12, 25)) + pm([1e-20, 3e-21, 1e-22]) + [0.0], [1e100, -1e-100],
                 0, 0, "two multiplies in T")
    # exp: down to where e^x is a Float32 subnormal (x < -87.3) and 0 (x < -103.3), up to overflow (88.72)
    R["exp"] = Unary(lambda x: mp.exp(x), span(-10, 10, 41) + span(-104, -80, 25) + span(80, 88.7, 10) + around(0.0, (0,)),
                [-745.0, -740.0, -708.0, 700.0, 709.5], 1, 0, "the rule is the value e^x itself")
    R["abs"] = Unary(lambda x: mp.sign(x), pm(geo(1e-40, 3e38, 27)), [], 0, 0, "sign(x), x != 0")
    logs = geo(F32_MIN, 1e38, 39) + around(1.0) + above(F32_MIN, (1, 2)) + span(0.5, 2, 13)
    # 5e-39 is a subnormal operand (1/x = 2e38 still finite in Float32)
    R["log"] = Unary(lambda x: 1 / x, logs + [5e-39, 3e38], [1e-300, 1e300], 0, 1, "1/x")
    R["log2"] = Unary(lambda x: 1 / (x * mp.log(2)), logs, [1e-300, 1e300], 0, 1, "ln 2 is a literal; one multiply, one divide")
    R["log10"] = Unary(lambda x: 1 / (x * mp.log(10)), logs, [1e-300, 1e300], 0, 1, "ln 10 is a literal")
    R["log1p"] = Unary(lambda x: 1 / (1 + x), above(-1.0, (1, 2, 16, 1024)) + around(0.0, (0,)) + pm(geo(1e-30, 0.9, 19))
                  + around(1.0) + geo(1.5, 1e38, 21) + [-0.999, -0.99], [1e300], 0, 1, "1/(1 + x); 1 + x is exact near -1")
    R["sqrt"] = Unary(lambda x: 1 / (2 * mp.sqrt(x)), geo(F32_MIN, 3e38, 41) + around(1.0) + [1e-40, 1e-44, 0.25, 4.0],
                 [1e-300, 1e300], 0, 1, "sqrt is correctly rounded: no transcendental")
    R["sin"] = Unary(lambda x: mp.cos(x), trig, [], 1, 0, "cos x")
    R["cos"] = Unary(lambda x: -mp.sin(x), trig + around(0.0, (0,)) + pm(geo(1e-30, 1e-3, 7)), [], 1, 0, "-sin x")
    # sec^2 x: near pi/2 the value (2e7 at the Float32 nearest pi/2) stays finite and so does sec^2
    R["tan"] = Unary(lambda x: 1 / mp.cos(x) ** 2, span(-1.5, 1.5, 31) + around(PI / 4) + pm(around(PI / 2, (-2, -1, 0, 1, 2)))
                + around(PI) + pm([10.0, 1e3, 1e5, 1.1e5, 1e8]) + pm(geo(1e-30, 1e-3, 5)), [], 2, 1,
                "2, because cos is squared; 1/c^2 divides")
    hyp = span(-10, 10, 41) + pm(geo(10, 88.5, 12)) + pm(geo(1e-30, 1e-3, 7)) + pm([1e-40])
    R["sinh"] = Unary(lambda x: mp.cosh(x), hyp, [700.0, -700.0, 709.0], 1, 0, "cosh x")
    # sinh(1e-40) = 1e-40 is a Float32 subnormal result
    R["cosh"] = Unary(lambda x: mp.sinh(x), hyp, [700.0, -700.0, 709.0], 1, 0, "sinh x")
    # 1 - tanh^2 cancels: an error of half an ulp of 1 in t^2 is 1/(1 - t^2) half-ulps of the result, and both
    # tables (and ForwardDiff's rule, 1 - tanh(x)^2) compute it this way. Narrowed by hand to |x| <= 1.25, where
    # 1 - t^2 >= 0.28 keeps the amplification below 4.
    R["tanh"] = Unary(lambda x: 1 / mp.cosh(x) ** 2, span(-1.25, 1.25, 41) + pm(geo(1e-30, 1e-2, 9)) + [0.0], [], 2, 0,
                 "2, because tanh is squared")
    # 1/(1 + x^2): x^2 must stay finite in T (|x| <= 1e19 in Float32): beyond, the rule gives 0 where the true
    # derivative is still a subnormal. Narrowed by hand; the reference squares x in T the same way.
    wide = pm(geo(1e-30, 1e18, 33)) + span(-3, 3, 25) + [0.0]
    R["atan"] = Unary(lambda x: 1 / (1 + x * x), wide, [1e150, -1e150], 0, 1, "1/(1 + x^2)")
    R["asinh"] = Unary(lambda x: 1 / mp.sqrt(x * x + 1), wide, [1e150, -1e150], 0, 1, "1/sqrt(x^2 + 1): sqrt is not transcendental")
    # 1/sqrt(x^2 - 1) cancels next to 1 when x^2 is rounded; at a Float32-representable operand x^2 - 1 is exact
    # in Float64 (both oracle evaluations form it there), so the grid starts one Float32 ulp above 1. The
    # Float32 engine rounds x^2: that is the operand's own conditioning (spread), not the rule's error.
    # acosh(1) itself is a convention (Inf).
    R["acosh"] = Unary(lambda x: 1 / mp.sqrt((x - 1) * (x + 1)), above(1.0) + span(1.0625, 3, 32) + geo(3, 1e18, 33), [1e150],
                  0, 1, "1/sqrt(x^2 - 1)")
    # atanh_clip(x) = atanh(mod(x + 1, 2) - 1), differentiated operator by operator: atanh'(u) = 1/(1 - u^2), and
    # the sum, the floored mod (slope 1 in its first argument) and the difference pass the tangent unchanged.
    # Operands are multiples of 2^-10 with |x| < 8, so x + 1 is exact in T and u is the operand atanh really sees;
    # odd integers (u = -1, an infinite value) are left out. 1 - u^2 = (1 - u)(1 + u) near |u| = 1 is exact here.
    ac = [k / 64 for k in range(-300, 301) if k % 64 != 0 or (k // 64) % 2 == 0]
    ac = [v for i, v in enumerate(ac) if i % 4 == 0 or abs(v) < 1.1]
    ac += [1 - 2.0 ** -10, -1 + 2.0 ** -10, 1 + 2.0 ** -10, 3 - 2.0 ** -10, -3 + 2.0 ** -10, 0.05 + 1.3, 0.05 + 2.7, 0.05 + 0.4]
    R["atanh_clip"] = Unary(lambda x: 1 / (1 - u_of(x) ** 2), ac, [], 0, 1, "1/(1 - u^2), u by exact operations")
    # 2/sqrt(pi) exp(-x^2): to |x| = 10.5 in Float32 (a subnormal from 9.3, 0 from 10.2) and 26.5 in Float64.
    # The rule (ForwardDiff's too) squares x in T, and a rounded x^2 alone would be x^2/2 ulps of the result:
    # operands beyond 4.5 are multiples of 1/8 (ERF_TAIL) whose square is exact in Float32, and every
    # Float32-representable operand has an exact square in Float64.
    erfg = span(-4.5, 4.5, 73) + pm(geo(1e-30, 1e-2, 7)) + [0.0] + ERF_TAIL
    erf64 = pm([12.0, 20.0, 26.0, 26.5])
    R["erf"] = Unary(lambda x: 2 / mp.sqrt(mp.pi) * mp.exp(-x * x), erfg, erf64, 1, 0, "exp(-x^2)")
    R["erfc"] = Unary(lambda x: -2 / mp.sqrt(mp.pi) * mp.exp(-x * x), erfg, erf64, 1, 0, "exp(-x^2)")
    R["relu"] = Unary(lambda x: one if x > 0 else 0 * one, pm(geo(1e-40, 1e38, 27)), [], 0, 0, "step, x != 0")
    # -1/x^2: x^2 must stay a normal number in T
    R["inv"] = Unary(lambda x: -1 / (x * x), pm(geo(1e-18, 1e18, 37)) + around(1.0) + around(-1.0), [1e-150, 1e150], 0, 1,
                "-1/x^2")
    # stored for the day the rule is provided (Γ(x)·ψ(x)); today the engine's rule is 0 (conv table, a deviation)
    R["gamma"] = Unary(lambda x: mp.gamma(x) * mp.digamma(x), span(0.125, 30, 60) + [-0.5, -1.5, -2.5, -3.75, 1.4616321],
                  [100.0, 170.0], 2, 0, "Γ and ψ")
    return R



# in-domain interval for the random rows that fill a batch after the grid (checked against the oracle only)
UNARY_FILL = {"log": (0.1, 10), "log2": (0.1, 10), "log10": (0.1, 10), "log1p": (-0.9, 10), "sqrt": (0.1, 10),
              "acosh": (1.1, 10), "atanh_clip": (-0.9, 0.9), "tan": (-1.2, 1.2), "gamma": (0.5, 5),
              "exp": (-5, 5), "sinh": (-5, 5), "cosh": (-5, 5), "inv": (0.5, 4), "tanh": (-1.2, 1.2)}
# The only grid points whose bound against the fixture is infinite (a 4-ulp move of the operand leaves the
# domain): stated here and nowhere else; such a point is still held to the oracle in T. Any other point
# without a finite conditioning term fails the generator.
INFINITE_SPREAD = {("acosh", "f32"): [1.0000001192092896, 1.000000238418579]}  # 1 and 2 Float32 ulps above 1
ZERO_UNARY = ["round", "floor", "ceil", "sign"]
ZERO_BINARY = ["greater", "logical_or", "logical_and"]


# ---- the binary rules. Partials that are conventions inside a block (pow's d/dy at
# x <= 0) are written as the convention (0) and carry no error.

def binary_rules(mp):
    one = mp.mpf(1)
    gen_a = [-3.5, -1.0, -0.25, 0.5, 1.0, 2.75, 1e10, -1e-10, 1e-20, 7.0, -1e5, 0.001]
    gen_b = [-2.5, -1.0, -0.125, 0.75, 1.0, 3.25, 1e9, -1e-9, 12.0]
    R = {}
    R["+"] = Binary(lambda x, y: one, lambda x, y: one, [(gen_a, gen_b)], (0, 0), (0, 0))
    R["-"] = Binary(lambda x, y: one, lambda x, y: -one, [(gen_a, gen_b)], (0, 0), (0, 0))
    R["*"] = Binary(lambda x, y: y, lambda x, y: x, [(gen_a, gen_b)], (0, 0), (0, 0))
    R["/"] = Binary(lambda x, y: 1 / y, lambda x, y: -x / (y * y), [(gen_a, gen_b)], (0, 0), (1, 1))
    # pow: positive bases with every exponent; negative bases and base 0 with integer exponents (d/dy at
    # x <= 0 is the convention 0); exponent 0 and 1 in every block; base 0 only with exponents >= 1
    # (0^0's d/dx is 0·0^-1, a convention, and a negative exponent has no finite value).
    pos = ([0.5, 1.0, 1.5, 2.0, 10.0, 1e-3, 0.999, 37.5], [-2.0, -1.0, 0.0, 0.5, 1.0, 2.0, 2.5, 3.0, -0.75, 7.0])
    neg = ([-2.0, -0.5, -1.0, -3.0, -10.0], [0.0, 1.0, 2.0, 3.0, -1.0, -2.0, 5.0])
    zero = ([0.0], [1.0, 2.0, 3.0])
    R["pow"] = Binary(lambda x, y: y * x ** (y - 1) if (x != 0 or y != 1) else one,
                     lambda x, y: x ** y * mp.log(x) if x > 0 else 0 * one, [pos, neg, zero], (1, 2), (0, 0),
                     # an integer exponent is exact in T and is what makes a base <= 0 legal: the conditioning
                     # of such a point is the base's alone (a moved exponent would leave the domain)
                     moves_y=lambda x, y: not (x <= 0 and y == int(y)))
    # mod(x, y) = x - y·floor(x/y): d/dx = 1, d/dy = -floor(x/y); mixed signs, quotients either exact
    # integers or far from one (so the rounding of x/y in T cannot move the floor)
    R["mod"] = Binary(lambda x, y: one, lambda x, y: -mp.floor(x / y),
                [([5.5, -5.5, 7.25, -7.25, 0.75, -0.75, 100.5, -100.5, 1e6 + 0.5, 0.0], [2.0, -2.0, 3.0, -3.0, 0.5, -0.5, 1.25, -1.25])],
                (0, 0), (0, 1))
    ma, mb = [-2.0, -0.0, 0.5, 3.0, 1e10, -1e10, 1e-30], [-1.0, 0.25, 2.0, 7.0, -1e-30, 1e20]
    R["max"] = Binary(lambda x, y: one if x > y else 0 * one, lambda x, y: one if y > x else 0 * one, [(ma, mb)], (0, 0), (0, 0))
    R["min"] = Binary(lambda x, y: one if x < y else 0 * one, lambda x, y: one if y < x else 0 * one, [(ma, mb)], (0, 0), (0, 0))
    # the piecewise-constant operators: 0 everywhere by convention (ties and the steps themselves included), kept
    # as a grid so that they pass through every tangent combination like the others
    za, zb = [-3.5, -1.0, 0.0, 0.5, 1.0, 2.75, 1e10, -1e-10], [-2.5, -1.0, 0.0, 0.5, 1.0, 3.25, 1e9]
    for name in ZERO_BINARY:
        R[name] = Binary(lambda x, y: 0 * one, lambda x, y: 0 * one, [(za, zb)], (0, 0), (0, 0))
    return R


# ---- conventions: (operator, x[, y], T or "both", expected class(es)) -----------------
# Classes: "0", "+inf", "-inf", "nan", or a number (exact). Written out by hand; where
# mathematics gives no answer the project follows the oracle (the reference's rules).

CONV_UNARY = [
    ("abs", 0.0, "both", "0"), ("abs", -0.0, "both", "0"),
    ("relu", 0.0, "both", "0"), ("relu", -0.0, "both", "0"),
    ("sqrt", 0.0, "both", "+inf"),      # value 0, slope infinite
    ("acosh", 1.0, "both", "+inf"),     # value 0, slope infinite
    # inv of a subnormal whose reciprocal is still finite (1/1.1e-38 = 9.1e37): x^2 = 0, so -Inf (the true
    # -8e75 overflows Float32 too)
    ("inv", 1.1e-38, "f32", "-inf"),
    ("inv", 1e-308, "f64", "-inf"),     # x = 1e-308: 1/x finite, -1/x^2 overflows
    ("gamma", 2.5, "both", "0"), ("gamma", 0.5, "both", "0"), ("gamma", -1.5, "both", "0"),  # DEVIATION: no digamma
] + [(op, x, "both", "0") for op in ZERO_UNARY for x in (-2.5, -0.5, -0.0, 0.0, 0.5, 1.0, 1.5, 2.5, 1e10, -3.0)]

DEVIATIONS = ["gamma"]

CONV_BINARY = [
    # ties: the left operand takes the derivative (x >= y, x <= y)
    ("max", 1.5, 1.5, "both", 1.0, "0"), ("min", 1.5, 1.5, "both", 1.0, "0"),
    ("max", 0.0, -0.0, "both", 1.0, "0"), ("min", 0.0, -0.0, "both", 1.0, "0"),
    ("max", -0.0, 0.0, "both", 1.0, "0"), ("min", -0.0, 0.0, "both", 1.0, "0"),
    # pow: d/dy is 0 wherever ln x does not exist (x <= 0)
    ("pow", -2.0, 3.0, "both", 12.0, "0"), ("pow", -2.0, 2.0, "both", -4.0, "0"), ("pow", 0.0, 2.0, "both", "0", "0"),
    ("pow", 0.0, 1.0, "both", 1.0, "0"),
    # 0 · 0^-1, and 0^-1 is NaN by safe_pow (the reference's 0 · Inf). d/dy is 0 by the rule but cannot be seen
    # alone: the oracle multiplies the NaN d/dx by the other operand's zero tangent ("-": not checked)
    ("pow", 0.0, 0.0, "both", "nan", "-"),
    ("pow", 1.0, 0.0, "both", "0", "0"),     # exponent 0: d/dx = 0 · 1^-1, d/dy = 1 · ln 1
] + [(op, x, y, "both", "0", "0") for op in ZERO_BINARY
     for x, y in ((1.0, 2.0), (2.0, 1.0), (1.0, 1.0), (0.0, 0.0), (-1.0, 0.5), (0.5, -1.0), (-1.0, -2.0), (0.0, 1.0))]


# ---- evaluation ----------------------------------------------------------------------

def ulp_of(t, T):
    """The spacing of T at |t| (t a Float64 array; the smallest subnormal below the normal range)."""
    fi = np.finfo(T)
    a = np.abs(np.asarray(t, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
        e = np.maximum(e, fi.minexp)
        return np.ldexp(1.0, (e - fi.nmant).astype(np.int64))


def ulp_err(got, true, T):
    """|got - true| in ulps of T at true; 0 where T rounds true to the Inf or NaN that got is."""
    got = np.asarray(got, dtype=np.float64)
    true = np.asarray(true, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        tT = true.astype(T).astype(np.float64)
        err = np.abs(got - true) / ulp_of(true, T)
    same = (got == tT) | (np.isnan(got) & np.isnan(tT))
    return np.where(same & ~np.isfinite(tT), 0.0, np.where(np.isfinite(err), err, np.inf))


def to_f64(v):
    """An mpmath number rounded once to Float64."""
    return float(v)


def unary_grid(name, rule, tname):
    """The Float32-rounded grid; Float64 adds its extra points as they are."""
    if tname == "f32":
        return np.unique(r32(rule.grid))
    return np.unique(np.concatenate([r32(rule.grid), np.asarray(rule.f64_extra, dtype=np.float64)]))


def moved(fn, *args):
    """fn at moved operands, NaN where the move leaves the domain."""
    try:
        v = fn(*args)
        return float(v) if not hasattr(v, "imag") or v.imag == 0 else np.nan
    except (ValueError, ZeroDivisionError, TypeError):
        return np.nan


def eval_unary(mp, fn, x, T):
    """(d, spread): spread is the largest move of d under a 4-ulp-of-T move of the operand, Inf where the
    move reaches a pole or leaves the domain."""
    eps4 = 4 * float(np.finfo(T).eps)
    d = np.array([to_f64(fn(mp.mpf(float(v)))) for v in x])
    sp = np.zeros_like(d)
    for s in (1 + eps4, 1 - eps4):
        dm = np.array([moved(fn, mp.mpf(float(v)) * mp.mpf(s)) for v in x])
        with np.errstate(invalid="ignore", over="ignore"):
            mv = np.abs(dm - d)
        sp = np.maximum(sp, np.where(np.isnan(mv), np.inf, mv))
    return d, sp


def oracle_unary(name, x, T, opts):
    import oracle
    import srhip
    from srhip import Node

    tree = opts.make_unary(name, opts.make_binary("+", Node(val=-0.0), Node("x1")))
    flat = srhip.flatten([tree], opts, dtype=T)
    k, a, c = flat.tree(0)
    with np.errstate(all="ignore"):
        v, g, ok = oracle.eval_grad_consts(k, a, c.astype(T), x[None, :].astype(T), 1, dtype=T)
    return v, g[0].astype(np.float64), ok


def oracle_binary(name, x, y, T, opts):
    import oracle
    import srhip
    from srhip import Node

    B = opts.make_binary
    tree = B(name, B("+", Node(val=-0.0), Node("x1")), B("+", Node(val=-0.0), Node("x2")))
    flat = srhip.flatten([tree], opts, dtype=T)
    k, a, c = flat.tree(0)
    with np.errstate(all="ignore"):
        v, g, ok = oracle.eval_grad_consts(k, a, c.astype(T), np.stack([x, y]).astype(T), 2, dtype=T)
    return v, g[0].astype(np.float64), g[1].astype(np.float64), ok


def all_options():
    import srhip

    sys.path.insert(0, str(Path(__file__).parent))
    from make_golden import ALL_BIN, ALL_UNA

    return srhip.Options(binary_operators=ALL_BIN, unary_operators=ALL_UNA)


def binary_points(rule, tname):
    xs, ys, bl = [], [], []
    for b, (A, Bv) in enumerate(rule.blocks):
        for a in r32(A):
            for c in r32(Bv):
                xs.append(a), ys.append(c), bl.append(b)
    return np.array(xs), np.array(ys), np.array(bl, dtype=np.int32)


def eval_binary(mp, rule, x, y, T):
    """(dx, sx, dy, sy): the partials and their spreads under 4-ulp-of-T moves of both operands (of x alone
    where rule.moves_y says so), Inf where a move leaves the domain."""
    eps4 = 4 * float(np.finfo(T).eps)
    out = []
    for fn in (rule.dx, rule.dy):
        d = np.array([to_f64(fn(mp.mpf(float(a)), mp.mpf(float(b)))) for a, b in zip(x, y)])
        sp = np.zeros_like(d)
        for sa in (1 + eps4, 1 - eps4):
            for sb in (1 + eps4, 1 - eps4):
                dm = np.array([moved(fn, mp.mpf(float(a)) * mp.mpf(sa), mp.mpf(float(b)) * mp.mpf(sb if rule.moves_y(a, b) else 1))
                               for a, b in zip(x, y)])
                with np.errstate(invalid="ignore", over="ignore"):
                    mv = np.abs(dm - d)
                sp = np.maximum(sp, np.where(np.isnan(mv), np.inf, mv))
        out += [d, sp]
    return out  # dx, sx, dy, sy


def generate(only=None):
    """The fixture as a dict of arrays (only: a set of "una/<op>" / "bin/<op>" names, for the subsample check)."""
    import mpmath as mp

    mp.mp.dps = 60
    opts = all_options()
    out, failed = {}, []  # every grid problem is reported, not only the first
    UR, BR = unary_rules(mp), binary_rules(mp)
    for name, rule in UR.items():
        if only is not None and f"una/{name}" not in only:
            continue
        out[f"una/{name}/ntrans"] = np.int32(rule.ntrans)
        out[f"una/{name}/div"] = np.int32(rule.div)
        for tname, T in TYPES.items():
            x = unary_grid(name, rule, tname)
            d, sp = eval_unary(mp, rule.d, x, T)
            pre = f"una/{name}/{tname}"
            assert len(x) <= MAX_ROWS, (name, tname, len(x))
            out[f"{pre}/x"], out[f"{pre}/d"], out[f"{pre}/spread"] = x, d, sp
            inf_at = sorted(float(v) for v in x[~np.isfinite(sp)])
            if inf_at != INFINITE_SPREAD.get((name, tname), []):
                failed.append(f"{name} {tname}: no finite conditioning term (no working bound) at x = {inf_at}")
            if name in DEVIATIONS:
                out[f"{pre}/oracle_err_ulp"] = np.float64(np.nan)  # the rule is not provided
                continue
            v, g, ok = oracle_unary(name, x, T, opts)
            if not ok:
                failed.append(f"{name} {tname}: a grid value is not finite in T: x = {x[~np.isfinite(v)]}")
            err = ulp_err(g, d, T)
            worst = int(np.argmax(err))
            if not err[worst] <= MAX_ORACLE_ULP:
                failed.append(f"{name} {tname}: the oracle's rule is {err[worst]:.3g} ulp off at x = {x[worst]!r}: "
                              f"got {g[worst]!r}, true {d[worst]!r}")
            out[f"{pre}/oracle_err_ulp"] = np.float64(err[worst])
    for name, rule in BR.items():
        if only is not None and f"bin/{name}" not in only:
            continue
        out[f"bin/{name}/ntrans"] = np.array(rule.ntrans, dtype=np.int32)
        out[f"bin/{name}/div"] = np.array(rule.div, dtype=np.int32)
        for tname, T in TYPES.items():
            x, y, bl = binary_points(rule, tname)
            assert np.bincount(bl).max() <= MAX_ROWS, (name, np.bincount(bl))
            dx, sx, dy, sy = eval_binary(mp, rule, x, y, T)
            pre = f"bin/{name}/{tname}"
            out.update({f"{pre}/x": x, f"{pre}/y": y, f"{pre}/block": bl, f"{pre}/dx": dx, f"{pre}/dy": dy,
                        f"{pre}/sx": sx, f"{pre}/sy": sy})
            for what, s_ in (("d/dx", sx), ("d/dy", sy)):
                if not np.isfinite(s_).all():
                    failed.append(f"{name} {tname} {what}: no finite conditioning term (no working bound) at "
                                  f"{list(zip(x[~np.isfinite(s_)], y[~np.isfinite(s_)]))}")
            v, gx, gy, ok = oracle_binary(name, x, y, T, opts)
            if not ok:
                failed.append(f"{name} {tname}: a grid value is not finite in T at "
                              f"{list(zip(x[~np.isfinite(v)], y[~np.isfinite(v)]))}")
            worst_of = []
            for what, g, d in (("d/dx", gx, dx), ("d/dy", gy, dy)):
                err = ulp_err(g, d, T)
                w = int(np.argmax(err))
                if not err[w] <= MAX_ORACLE_ULP:
                    failed.append(f"{name} {tname} {what}: the oracle's rule is {err[w]:.3g} ulp off at "
                                  f"({x[w]!r}, {y[w]!r}): got {g[w]!r}, true {d[w]!r}")
                worst_of.append(err[w])
            out[f"{pre}/oracle_err_ulp"] = np.array(worst_of)
    if failed:
        raise SystemExit("\n".join(failed))
    if only is None:
        for name in UNARY_FILL:
            out[f"fill/{name}"] = np.array(UNARY_FILL[name], dtype=np.float64)
        cu = CONV_UNARY
        out["conv/una/op"] = np.array([c[0] for c in cu], dtype="U16")
        out["conv/una/x"] = np.array([c[1] for c in cu], dtype=np.float64)
        out["conv/una/T"] = np.array([c[2] for c in cu], dtype="U8")
        out["conv/una/cls"] = np.array([str(c[3]) for c in cu], dtype="U32")
        cb = CONV_BINARY
        out["conv/bin/op"] = np.array([c[0] for c in cb], dtype="U16")
        out["conv/bin/x"] = np.array([c[1] for c in cb], dtype=np.float64)
        out["conv/bin/y"] = np.array([c[2] for c in cb], dtype=np.float64)
        out["conv/bin/T"] = np.array([c[3] for c in cb], dtype="U8")
        out["conv/bin/cls_dx"] = np.array([repr(c[4]) if not isinstance(c[4], str) else c[4] for c in cb], dtype="U32")
        out["conv/bin/cls_dy"] = np.array([repr(c[5]) if not isinstance(c[5], str) else c[5] for c in cb], dtype="U32")
        out["conv/deviations"] = np.array(DEVIATIONS, dtype="U16")
        out["zero/una"] = np.array(ZERO_UNARY, dtype="U16")
        out["zero/bin"] = np.array(ZERO_BINARY, dtype="U16")
    return out


def main():
    out = generate()
    path = Path(__file__).with_name("derivatives.npz")
    np.savez_compressed(path, **out)
    npts = sum(v.size for k, v in out.items() if k.endswith("/x") and not k.startswith("conv"))
    print("wrote", len(out), "arrays,", npts, "points,", path.stat().st_size, "bytes")
    for k in sorted(out):
        if k.endswith("oracle_err_ulp"):
            print(f"  {k:40s} {np.round(out[k], 3)}")


if __name__ == "__main__":
    main()
