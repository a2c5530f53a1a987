"""Generate tests/golden/second_derivatives.npz — an independent reference for every
operator's second-order rule (device_ops.h uop_d2 / bop_d2; run by hand on the CPU:
python tests/golden/make_second_derivative_golden.py; needs mpmath 1.3).

Closed-form f'' and fxx / fxy / fyy from the mathematics (from neither device table),
evaluated by mpmath at 60 digits at the exact operand and rounded once to Float64, on the
operand grids of make_derivative_golden.py (imported). A grid is narrowed by hand below,
with the reason, where the second derivative — or an intermediate of the rule as written,
which is the first-order rule differentiated — leaves T although the first did not.

Stored per unary operator `una/<op>/<T>/`: x, d2, spread (the movement of d2 under a
4-ulp-of-T move of the operand), rule_err_ulp (below); `una/<op>/ntrans`, `una/<op>/div`.
Per binary operator `bin/<op>/<T>/`: x, y, block, dxx, dxy, dyy, sxx, sxy, syy,
rule_err_ulp (3); `bin/<op>/ntrans`, `bin/<op>/div` (3 each).
`conv/...`: the convention points with hand-written classes.

rule_err_ulp takes the place of the first-order fixture's oracle_err_ulp (the C oracle has
no second-order rules): the worst error, in ulps of T of the true value, of the rule AS
WRITTEN evaluated in T arithmetic with every transcendental value correctly rounded (mpmath
rounded to T). It is the rule's own rounding and cancellation, computed here and never
from the engine. The test's bound adds 4 ulp per transcendental value that enters the rule
multiplicatively (`ntrans`: the engine's are not correctly rounded) and 2 ulp per divide or
reciprocal (`div`), as tests/test_derivative_rules_gpu.py does, plus the conditioning.
Every point must stay within MAX_RULE_ULP or the generator fails naming it.
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
spec = importlib.util.spec_from_file_location("make_derivative_golden", HERE / "make_derivative_golden.py")
G1 = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G1)

MAX_RULE_ULP = 16.0
TYPES = G1.TYPES
LN2, LN10 = 0.69314718055994530942, 2.30258509299404568402
SQPI2 = 1.1283791670955126


def second_unary(mp):
    """op -> (closed-form f'', ntrans, div, keep(x, T) or None: the narrowing, reason)."""
    def u_of(x):
        s = x + 1
        return s - 2 * mp.floor(s / 2) - 1

    one = mp.mpf(1)
    R = {}
    R["neg"] = (lambda x: 0 * one, 0, 0, None, "")
    R["square"] = (lambda x: 2 * one, 0, 0, None, "")
    R["cube"] = (lambda x: 6 * x, 0, 0, None, "")
    R["exp"] = (lambda x: mp.exp(x), 1, 0, None, "")
    R["abs"] = (lambda x: 0 * one, 0, 0, None, "")
    # -(f1·f1), f1 = 1/x: exact powers of the first rule
    R["log"] = (lambda x: -1 / (x * x), 0, 1, None, "")
    R["log2"] = (lambda x: -1 / (x * x * mp.log(2)), 0, 2, None, "")
    R["log10"] = (lambda x: -1 / (x * x * mp.log(10)), 0, 2, None, "")
    R["log1p"] = (lambda x: -1 / ((1 + x) ** 2), 0, 1, None, "")
    R["sqrt"] = (lambda x: -1 / (4 * x * mp.sqrt(x)), 0, 2, None, "")
    R["sin"] = (lambda x: -mp.sin(x), 1, 0, None, "")
    R["cos"] = (lambda x: -mp.cos(x), 1, 0, None, "")
    # 2·tan·sec²: next to pi/2 tan and sec² are ~1e7 and 1e15 with relative error ~1e8 ulp of the operand's
    # rounding already in the value (the first rule's grid kept them because sec² alone stays finite);
    # the product squares that. Narrowed to |cos x| >= 1e-3.
    R["tan"] = (lambda x: 2 * mp.tan(x) / mp.cos(x) ** 2, 3, 1, lambda x, T: abs(np.cos(x)) >= 1e-3,
                "|cos x| >= 1e-3")
    R["sinh"] = (lambda x: mp.sinh(x), 1, 0, None, "")
    R["cosh"] = (lambda x: mp.cosh(x), 1, 0, None, "")
    R["tanh"] = (lambda x: -2 * mp.tanh(x) / mp.cosh(x) ** 2, 3, 0, None, "")
    # -2x·f1², f1 = 1/(1 + x²): f1² must stay a normal number in T (the first rule needed only x² finite), so
    # |x| <= 1e9 in Float32, 1e75 in Float64. Beyond, the rule gives 0 where the true value is still representable.
    R["atan"] = (lambda x: -2 * x / (1 + x * x) ** 2, 0, 2, lambda x, T: abs(x) <= (1e9 if T == np.float32 else 1e75),
                 "f1² normal in T")
    R["asinh"] = (lambda x: -x / mp.sqrt(x * x + 1) ** 3, 0, 3, None, "")
    # -x·f1³ with f1 = 1/sqrt(x² − 1): the cube triples the first rule's conditioning next to 1, where its two
    # nearest Float32 operands already had no finite bound. Narrowed to x >= 1.0625.
    R["acosh"] = (lambda x: -x / mp.sqrt((x - 1) * (x + 1)) ** 3, 0, 3, lambda x, T: x >= 1.0625, "x >= 1.0625")
    R["atanh_clip"] = (lambda x: 2 * u_of(x) / (1 - u_of(x) ** 2) ** 2, 0, 2, None, "")
    R["erf"] = (lambda x: -4 * x / mp.sqrt(mp.pi) * mp.exp(-x * x), 1, 0, None, "")
    R["erfc"] = (lambda x: 4 * x / mp.sqrt(mp.pi) * mp.exp(-x * x), 1, 0, None, "")
    R["relu"] = (lambda x: 0 * one, 0, 0, None, "")
    R["inv"] = (lambda x: 2 / (x * x * x), 0, 2, None, "")
    return R


def emulate_unary(op, x, T, mp):
    """The rule as written (uop_d2) in T arithmetic, transcendental values correctly rounded."""
    t = T

    def cr(fn, v):  # correctly rounded transcendental of a T value
        with np.errstate(over="ignore"):
            return np.asarray([float(fn(mp.mpf(float(a)))) for a in v], dtype=np.float64).astype(t)

    x = x.astype(t)
    with np.errstate(all="ignore"):
        if op in ("neg", "abs", "relu"):
            return np.zeros_like(x)
        if op == "square":
            return np.full_like(x, 2)
        if op == "cube":
            return t(6) * x
        if op == "exp":
            return cr(mp.exp, x)
        if op == "log":
            f1 = t(1) / x
            return -(f1 * f1)
        if op in ("log2", "log10"):
            f1 = t(1) / (x * t(LN2 if op == "log2" else LN10))
            return -f1 / x
        if op == "log1p":
            f1 = t(1) / (t(1) + x)
            return -(f1 * f1)
        if op == "sqrt":
            f1 = t(0.5) / np.sqrt(x)
            return t(-0.5) * f1 / x
        if op == "sin":
            return -cr(mp.sin, x)
        if op == "cos":
            return -cr(mp.cos, x)
        if op == "tan":
            c = cr(mp.cos, x)
            return t(2) * cr(mp.tan, x) * (t(1) / (c * c))
        if op == "sinh":
            return cr(mp.sinh, x)
        if op == "cosh":
            return cr(mp.cosh, x)
        if op == "tanh":
            f = cr(mp.tanh, x)
            return t(-2) * f * (t(1) - f * f)
        if op == "atan":
            f1 = t(1) / (t(1) + x * x)
            return t(-2) * x * (f1 * f1)
        if op in ("asinh", "acosh"):
            f1 = t(1) / np.sqrt(x * x + (t(1) if op == "asinh" else t(-1)))
            return -x * (f1 * f1) * f1
        if op == "atanh_clip":
            s = x + t(1)
            u = (s - t(2) * np.floor(s / t(2))) - t(1)
            f1 = t(1) / (t(1) - u * u)
            return t(2) * u * (f1 * f1)
        if op in ("erf", "erfc"):
            f1 = t(SQPI2 if op == "erf" else -SQPI2) * cr(mp.exp, -x * x)
            return t(-2) * x * f1
        if op == "inv":
            return t(-2) * (t(-1) / (x * x)) * (t(1) / x)
    raise KeyError(op)


def second_binary(mp):
    """op -> (fxx, fxy, fyy, ntrans (3), div (3))."""
    one = mp.mpf(1)
    z = lambda x, y: 0 * one
    R = {name: (z, z, z, (0, 0, 0), (0, 0, 0)) for name in ["+", "-", "mod", "max", "min"] + G1.ZERO_BINARY}
    R["*"] = (z, lambda x, y: one, z, (0, 0, 0), (0, 0, 0))
    R["/"] = (z, lambda x, y: -1 / (y * y), lambda x, y: 2 * x / (y * y * y), (0, 0, 0), (0, 1, 2))
    # pow at x <= 0: fxy = fyy = 0 (the convention beside bop_d's fy = 0 branch); fxx = y(y-1)x^(y-2) with
    # 0^0 = 1 and 0·0^-1 left to the convention table
    R["pow"] = (lambda x, y: y * (y - 1) * x ** (y - 2) if x != 0 or y >= 2 else mp.nan,  # (0, 1): 1·0·0^-1, NaN by safe_pow
                lambda x, y: x ** (y - 1) * (1 + y * mp.log(x)) if x > 0 else 0 * one,
                lambda x, y: x ** y * mp.log(x) ** 2 if x > 0 else 0 * one, (1, 3, 3), (0, 0, 0))
    return R


def emulate_binary(op, x, y, T, mp):
    t = T
    x, y = x.astype(t), y.astype(t)
    zero = np.zeros_like(x)

    def cr2(fn, a, b):
        out = []
        for p, q in zip(a, b):
            try:
                v = fn(mp.mpf(float(p)), mp.mpf(float(q)))
                out.append(float(v) if not hasattr(v, "imag") or v.imag == 0 else np.nan)
            except (ValueError, ZeroDivisionError):
                out.append(np.nan)
        with np.errstate(over="ignore"):
            return np.asarray(out, dtype=np.float64).astype(t)

    with np.errstate(all="ignore"):
        if op == "*":
            return zero, np.ones_like(x), zero
        if op == "/":
            fx = t(1) / y
            fy = (-(x / y) * fx) if t == np.float32 else (-x / (y * y))
            return zero, -(fx * fx), t(-2) * fy * fx
        if op == "pow":
            pw = lambda a, b: cr2(lambda p, q: p ** q, a, b)
            f, p1, p2 = pw(x, y), pw(x, y - t(1)), pw(x, y - t(2))
            lx = cr2(lambda p, q: mp.log(p) if p > 0 else 0 * p, x, y)
            fx = y * p1
            fy = np.where(x > 0, f * lx, 0)
            fxx = y * (y - t(1)) * p2
            return fxx, np.where(x > 0, p1 + fx * lx, 0).astype(t), np.where(x > 0, fy * lx, 0).astype(t)
    return zero, zero, zero


# ---- conventions: hand-written classes -------------------------------------------------------
CONV_UNARY = [
    ("abs", 0.0, "both", "0"), ("abs", -0.0, "both", "0"), ("relu", 0.0, "both", "0"),
    # f1 = +Inf, f2 = -Inf, and the propagation adds f1·dxc = Inf · 0 (the operand's own mixed partial is 0):
    # NaN, as a zero first-order tangent under an infinite slope already is
    ("sqrt", 0.0, "both", "nan"),
    ("gamma", 2.5, "both", "0"), ("gamma", 0.5, "both", "0"),  # DEVIATION: the first rule is not provided
    ("inv", 1.1e-38, "f32", "nan"),    # x² = 0: f1 = -Inf, f2 = +Inf, and f1·dxc = -Inf · 0
] + [(op, x, "both", "0") for op in G1.ZERO_UNARY for x in (-2.5, -0.5, 0.0, 0.5, 1.5, 1e10)]

# (op, x, y, T, class of fxx, fxy, fyy); "-": not checked
CONV_BINARY = [
    ("pow", -2.0, 3.0, "both", -12.0, "0", "0"),   # x <= 0: fy = 0 is a constant branch, so fxy = fyy = 0
    ("pow", -2.0, 2.0, "both", 2.0, "0", "0"),
    ("pow", 0.0, 2.0, "both", 2.0, "0", "0"),      # 2·1·0^0
    ("pow", 0.0, 3.0, "both", "0", "0", "0"),
    ("pow", 0.0, 1.0, "both", "nan", "0", "0"),    # 1·0·0^-1: safe_pow refuses 0^-1 (0 · NaN)
    ("max", 1.5, 1.5, "both", "0", "0", "0"), ("min", -0.0, 0.0, "both", "0", "0", "0"),
    ("mod", 5.5, 2.0, "both", "0", "0", "0"), ("mod", -7.25, 3.0, "both", "0", "0", "0"),
] + [(op, x, y, "both", "0", "0", "0") for op in G1.ZERO_BINARY for x, y in ((1.0, 2.0), (2.0, 1.0), (0.0, 0.0), (-1.0, 0.5))]


def spread_of(fn, args_list, T, mp, moves):
    eps4 = 4 * float(np.finfo(T).eps)
    d = np.array([G1.to_f64(fn(*[mp.mpf(float(a)) for a in args])) for args in args_list])
    sp = np.zeros_like(d)
    scales = [(1 + eps4,), (1 - eps4,)] if len(args_list[0]) == 1 else [(a, b) for a in (1 + eps4, 1 - eps4) for b in (1 + eps4, 1 - eps4)]
    for sc in scales:
        dm = []
        for args in args_list:
            mv = [mp.mpf(float(a)) * mp.mpf(s if (i == 0 or moves(*args)) else 1) for i, (a, s) in enumerate(zip(args, sc))]
            dm.append(G1.moved(fn, *mv))
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.abs(np.array(dm) - d)
        sp = np.maximum(sp, np.where(np.isnan(m), np.inf, m))
    return d, np.where(np.isnan(d), 0.0, sp)  # (a NaN by convention has no conditioning)


def generate(only=None):
    import mpmath as mp

    mp.mp.dps = 60
    out, failed = {}, []
    U1, B1 = G1.unary_rules(mp), G1.binary_rules(mp)
    for name, (fn, ntrans, div, keep, reason) in second_unary(mp).items():
        if only is not None and f"una/{name}" not in only:
            continue
        out[f"una/{name}/ntrans"], out[f"una/{name}/div"] = np.int32(ntrans), np.int32(div)
        for tn, T in TYPES.items():
            x = G1.unary_grid(name, U1[name], tn)
            if keep is not None:
                x = x[[bool(keep(v, T)) for v in x]]
            d, sp = spread_of(fn, [(v,) for v in x], T, mp, lambda *a: True)
            # a point whose move leaves the domain has no working bound: dropped here, by rule, never at test time
            fin = np.isfinite(sp)
            if (~fin).sum() > 4:
                failed.append(f"{name} {tn}: {int((~fin).sum())} points without a finite conditioning term")
            x, d, sp = x[fin], d[fin], sp[fin]
            err = G1.ulp_err(emulate_unary(name, x, T, mp).astype(np.float64), d, T)
            # the rule's conditioning is not its error: a point is held to the bound plus 4·spread in the test, and
            # here to MAX_RULE_ULP plus that movement in ulps
            slack = 4 * sp / G1.ulp_of(d, T)
            w = int(np.argmax(err - slack))
            if not err[w] - slack[w] <= MAX_RULE_ULP:
                failed.append(f"{name} {tn}: the rule as written is {err[w]:.3g} ulp off at x = {x[w]!r} (slack {slack[w]:.3g})")
            pre = f"una/{name}/{tn}"
            out[f"{pre}/x"], out[f"{pre}/d2"], out[f"{pre}/spread"] = x, d, sp
            out[f"{pre}/rule_err_ulp"] = np.float64(np.max(np.maximum(err - slack, 0.0)))
    for name, (fxx, fxy, fyy, ntrans, div) in second_binary(mp).items():
        if only is not None and f"bin/{name}" not in only:
            continue
        out[f"bin/{name}/ntrans"], out[f"bin/{name}/div"] = np.array(ntrans, dtype=np.int32), np.array(div, dtype=np.int32)
        rule = B1[name]
        for tn, T in TYPES.items():
            x, y, bl = G1.binary_points(rule, tn)
            pre = f"bin/{name}/{tn}"
            out.update({f"{pre}/x": x, f"{pre}/y": y, f"{pre}/block": bl})
            em = emulate_binary(name, x, y, T, mp)
            worst = []
            for key, fn, e in (("xx", fxx, em[0]), ("xy", fxy, em[1]), ("yy", fyy, em[2])):
                d, sp = spread_of(fn, list(zip(x, y)), T, mp, rule.moves_y)
                if not np.isfinite(sp).all():
                    failed.append(f"{name} {tn} f{key}: no finite conditioning term at {list(zip(x[~np.isfinite(sp)], y[~np.isfinite(sp)]))}")
                    sp = np.where(np.isfinite(sp), sp, 0.0)
                out[f"{pre}/d{key}"], out[f"{pre}/s{key}"] = d, sp
                err = G1.ulp_err(e.astype(np.float64), d, T)
                slack = 4 * sp / G1.ulp_of(d, T)
                w = int(np.argmax(err - slack))
                if not err[w] - slack[w] <= MAX_RULE_ULP:
                    failed.append(f"{name} {tn} f{key}: the rule as written is {err[w]:.3g} ulp off at ({x[w]!r}, {y[w]!r})")
                worst.append(np.max(np.maximum(err - slack, 0.0)))
            out[f"{pre}/rule_err_ulp"] = np.array(worst)
    if failed:
        raise SystemExit("\n".join(failed))
    if only is None:
        out["conv/una/op"] = np.array([c[0] for c in CONV_UNARY], dtype="U16")
        out["conv/una/x"] = np.array([c[1] for c in CONV_UNARY], dtype=np.float64)
        out["conv/una/T"] = np.array([c[2] for c in CONV_UNARY], dtype="U8")
        out["conv/una/cls"] = np.array([str(c[3]) for c in CONV_UNARY], dtype="U32")
        out["conv/bin/op"] = np.array([c[0] for c in CONV_BINARY], dtype="U16")
        out["conv/bin/x"] = np.array([c[1] for c in CONV_BINARY], dtype=np.float64)
        out["conv/bin/y"] = np.array([c[2] for c in CONV_BINARY], dtype=np.float64)
        out["conv/bin/T"] = np.array([c[3] for c in CONV_BINARY], dtype="U8")
        for k, name in ((4, "xx"), (5, "xy"), (6, "yy")):
            out[f"conv/bin/cls_{name}"] = np.array([c[k] if isinstance(c[k], str) else repr(c[k]) for c in CONV_BINARY], dtype="U32")
    return out


def main():
    out = generate()
    path = HERE / "second_derivatives.npz"
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", path.stat().st_size, "bytes")
    for k in sorted(out):
        if k.endswith("rule_err_ulp"):
            print(f"  {k:40s} {np.round(out[k], 3)}")


if __name__ == "__main__":
    main()
