"""Writes tests/golden/losses.npz: every elementwise loss's per-row value ℓ(u) and derivative ℓ'(u) on a
hand-written grid, from mpmath at 80 digits. u is the residual r = ŷ - y of a distance loss and the agreement
a = y·ŷ of a margin loss. The closed forms are written from the mathematical definitions of the reference's
docs/src/losses.md (the line of every definition is in CONFIGS) and the table of include/srhip.h; none of the
engine's or the oracle's code is used or imported.

Per configuration and dtype, `<config>/<T>/`:
  u                 the grid (Float64 holding values of T), both signs;
  v_hi, v_lo        ℓ(u): RN_Float64 of the true value and (true - v_hi) in Float64 ulps of v_hi;
  d_hi, d_lo        ℓ'(u) likewise;
  v_rn, d_rn        RN_T of the true values (±Inf where T overflows);
  v_du, d_du        conditioning with respect to u: the largest move of the true value when u moves by half an
                    ulp of T (absolute; 0 for the algebraic losses, whose bound has no such term);
  v_dp, d_dp        conditioning with respect to the Float64 parameter: the move under one Float64 rounding of p
                    (LPDistLoss's p) or three of k = 2π/c (PeriodicLoss: 2π, the division, r·k);
  v_form, d_form    form-limited points (FORM below): the reference's verdict, NaN elsewhere;
  v_conv, d_conv    convention points (CONVENTIONS below): the written verdict, matched exactly; a point that
                    is none has the filler 12345.0 there.
`conv/*` is the convention table itself, `form/*` the form-limited one.

The generator asserts that every point that is neither has a finite bound (finite true value or a definite
RN_T = ±Inf, finite conditioning) and that form-limited points are at most 10 % of any grid.

    python tests/golden/make_loss_golden.py        # needs mpmath
"""
from pathlib import Path

import numpy as np

DPS = 80
NOT_CONV = 12345.0
TNAMES = {"f32": np.float32, "f64": np.float64}

# (config, SRHIP_LOSS name, parameter, kind, docs/src/losses.md line of the definition)
CONFIGS = [
    ("L2", "L2", None, "dist", 64), ("L1", "L1", None, "dist", 37),
    ("LP_0.5", "LP", 0.5, "dist", 28), ("LP_1.7", "LP", 1.7, "dist", 28),
    ("LPINT_2", "LPINT", 2.0, "dist", 28), ("LPINT_3", "LPINT", 3.0, "dist", 28), ("LPINT_4", "LPINT", 4.0, "dist", 28),
    ("LPINT_-2", "LPINT", -2.0, "dist", 28),
    ("HUBER_0.8", "HUBER", 0.8, "dist", 99), ("L1EPSINS_0.3", "L1EPSINS", 0.3, "dist", 127),
    ("L2EPSINS_0.3", "L2EPSINS", 0.3, "dist", 154), ("QUANTILE_0.3", "QUANTILE", 0.3, "dist", 206),
    ("PERIODIC_2.0", "PERIODIC", 2.0, "dist", 88), ("LOGCOSH", "LOGCOSH", None, "dist", 0),
    ("LOGITDIST", "LOGITDIST", None, "dist", 179),
    ("ZEROONE", "ZEROONE", None, "margin", 242), ("PERCEPTRON", "PERCEPTRON", None, "margin", 268),
    ("LOGITMARGIN", "LOGITMARGIN", None, "margin", 293), ("L1HINGE", "L1HINGE", None, "margin", 319),
    ("L2HINGE", "L2HINGE", None, "margin", 346), ("SMOOTHEDL1HINGE_0.5", "SMOOTHEDL1HINGE", 0.5, "margin", 371),
    ("SMOOTHEDL1HINGE_2.0", "SMOOTHEDL1HINGE", 2.0, "margin", 371), ("MODHUBER", "MODHUBER", None, "margin", 397),
    ("L2MARGIN", "L2MARGIN", None, "margin", 423), ("EXP", "EXP", None, "margin", 450),
    ("SIGMOID", "SIGMOID", None, "margin", 476), ("DWDMARGIN_1.0", "DWDMARGIN", 1.0, "margin", 503),
    ("DWDMARGIN_3.0", "DWDMARGIN", 3.0, "margin", 503),
]
# the losses whose bound has an OCML figure and conditioning terms; every other one is algebraic
TRANSCENDENTAL = ("LP", "LOGCOSH", "LOGITDIST", "LOGITMARGIN", "EXP", "PERIODIC", "SIGMOID")
CW_COS_MAX = 1.6e6  # device_ops.h kCwCosMax, the Float32 Periodic routine's range in |r·k|


def neighbours(c, T, ks=(-2, -1, 0, 1, 2)):
    """The value of T nearest c moved by k ulps of T."""
    out = []
    for k in ks:
        v = T(c)
        for _ in range(abs(k)):
            v = np.nextafter(v, T(np.inf if k > 0 else -np.inf))
        out.append(float(v))
    return out


def magnitudes(cfg, name, p, kind, T):
    """The hand-written grid of |u| for one configuration (signs are added by grid())."""
    fi = np.finfo(T)
    f32 = T is np.float32
    m = [0.0, float(fi.smallest_subnormal), float(fi.tiny)]
    m += [2.0 ** -k for k in ((24, 21, 18, 15, 12, 10, 8, 6, 4, 2, 1) if f32 else (50, 43, 36, 30, 24, 21, 18, 15, 12, 10, 8, 6, 4, 2, 1))]
    m += [1.0, 10.0, 44.0, 88.0, 89.0, 160.0, 161.0, 709.0, 710.0, 1e4]
    if name in ("L2", "LPINT"):  # where the square leaves T
        m += neighbours(np.sqrt(np.float64(fi.max)), T, (-1, 0, 1))
    if name in ("HUBER", "L1EPSINS", "L2EPSINS"):
        m += neighbours(p, T)
    if name == "PERIODIC":  # multiples of c/4, both sides of the Float32 routine's range, far beyond it
        m += [0.25 * p, 0.75 * p, p, 1.5 * p, 509295.0, 509297.0, 1e7]
        assert 509295.0 * 2 * np.pi / p < CW_COS_MAX < 509297.0 * 2 * np.pi / p
    if kind == "margin":
        m += neighbours(1.0, T, (-2, -1, 1, 2))  # the hinge at 1 (ModHuber's other kink is -1: the negative side)
        m += [2.0, 3.0, 5.0, 20.0]  # where the smooth margin losses still move
        if name == "SMOOTHEDL1HINGE":
            m += neighbours(abs(1.0 - p), T) if p != 1.0 else []
        if name == "DWDMARGIN":
            m += neighbours(p / (p + 1.0), T)
    return sorted(set(float(T(v)) for v in m))


def grid(cfg, name, p, kind, T):
    m = magnitudes(cfg, name, p, kind, T)
    u = [s * v for v in m for s in (1.0, -1.0)]  # +0.0 and -0.0 both
    return np.array(u, dtype=np.float64)


# ---- the definitions, in mpmath ------------------------------------------------------------------

def definitions(mp):
    mpf = mp.mpf

    def sign(r):
        return mpf(1) if r > 0 else (mpf(-1) if r < 0 else mpf(0))

    def lncosh(r):
        a = abs(r)
        return mp.log(mp.cosh(a)) if a < 1 else a + mp.log1p(mp.exp(-2 * a)) - mp.log(2)

    def hinge(a):
        return max(mpf(0), 1 - a)

    def value(name, p, u):
        """ℓ(u), or None where the definition has no value (a division by zero)."""
        a = abs(u)
        if name == "L2": return u * u
        if name == "L1": return a
        if name in ("LP", "LPINT"):
            if a == 0:
                return mpf(0) if p > 0 else None
            return a ** p
        if name == "HUBER": return u * u / 2 if a <= p else p * (a - p / 2)
        if name == "L1EPSINS": return max(mpf(0), a - p)
        if name == "L2EPSINS": return max(mpf(0), a - p) ** 2
        if name == "QUANTILE": return p * u if u >= 0 else (p - 1) * u
        if name == "PERIODIC": return 1 - mp.cos(2 * mp.pi * u / p)
        if name == "LOGCOSH": return lncosh(u)
        if name == "LOGITDIST": return 2 * lncosh(u / 2)  # -ln(4 e^r / (1 + e^r)^2)
        if name == "ZEROONE": return mpf(1) if u < 0 else mpf(0)
        if name == "PERCEPTRON": return max(mpf(0), -u)
        if name == "LOGITMARGIN": return mp.log1p(mp.exp(-u)) if u > -50 else -u + mp.log1p(mp.exp(u))
        if name == "L1HINGE": return hinge(u)
        if name == "L2HINGE": return hinge(u) ** 2
        if name == "SMOOTHEDL1HINGE": return hinge(u) ** 2 / (2 * p) if u >= 1 - p else 1 - p / 2 - u
        if name == "MODHUBER": return hinge(u) ** 2 if u >= -1 else -4 * u
        if name == "L2MARGIN": return (1 - u) ** 2
        if name == "EXP": return mp.exp(-u)
        if name == "SIGMOID": return 1 - mp.tanh(u)
        if name == "DWDMARGIN":
            if u >= p / (p + 1):
                return 1 - u
            return None if u == 0 else (p ** p / (p + 1) ** (p + 1)) / u ** p
        raise KeyError(name)

    def deriv(name, p, u):
        a = abs(u)
        if name == "L2": return 2 * u
        if name == "L1": return sign(u)
        if name in ("LP", "LPINT"):
            if a == 0:
                return mpf(0) if p > 1 else None  # p < 1: Inf · 0
            return p * a ** (p - 1) * sign(u)
        if name == "HUBER": return u if a <= p else p * sign(u)
        if name == "L1EPSINS": return sign(u) if a > p else mpf(0)
        if name == "L2EPSINS": return 2 * (a - p) * sign(u) if a > p else mpf(0)
        if name == "QUANTILE": return p if u >= 0 else p - 1
        if name == "PERIODIC":
            k = 2 * mp.pi / p
            return k * mp.sin(k * u)
        if name == "LOGCOSH": return mp.tanh(u)
        if name == "LOGITDIST": return mp.tanh(u / 2)
        if name == "ZEROONE": return mpf(0)
        if name == "PERCEPTRON": return mpf(0) if u >= 0 else mpf(-1)
        if name == "LOGITMARGIN": return -1 / (1 + mp.exp(u))
        if name == "L1HINGE": return mpf(0) if u >= 1 else mpf(-1)
        if name == "L2HINGE": return mpf(0) if u >= 1 else 2 * (u - 1)
        if name == "SMOOTHEDL1HINGE": return (mpf(0) if u >= 1 else (u - 1) / p) if u >= 1 - p else mpf(-1)
        if name == "MODHUBER": return (mpf(0) if u > 1 else 2 * (u - 1)) if u >= -1 else mpf(-4)
        if name == "L2MARGIN": return 2 * (u - 1)
        if name == "EXP": return -mp.exp(-u)
        if name == "SIGMOID": return -1 / mp.cosh(u) ** 2
        if name == "DWDMARGIN":
            s = p / (p + 1)
            if u >= s:
                return mpf(-1)
            return None if u == 0 else -(s ** (p + 1)) / u ** (p + 1)
        raise KeyError(name)

    return value, deriv


# ---- the convention table: the discrete verdicts a Julia user sees --------------------------------
# (config, u, "v" or "d", the verdict, where it is written). "nan" and "inf" are verdicts too.
CONVENTIONS = [
    ("L1", 0.0, "d", 0.0, "losses.md:37: sign(0) = 0 at +0"), ("L1", -0.0, "d", 0.0, "losses.md:37: sign(-0) = 0"),
    ("QUANTILE_0.3", 0.0, "d", 0.3, "losses.md:206: r >= 0 takes tau at +0"),
    ("QUANTILE_0.3", -0.0, "d", 0.3, "losses.md:206: -0 >= 0, tau too"),
    ("QUANTILE_0.3", 0.0, "v", 0.0, "losses.md:206"), ("QUANTILE_0.3", -0.0, "v", 0.0, "losses.md:206"),
    ("L1EPSINS_0.3", "p", "d", 0.0, "losses.md:127: |r| > eps, not >=: the slope at |r| = eps is 0"),
    ("L1EPSINS_0.3", "-p", "d", 0.0, "losses.md:127"),
    ("L1EPSINS_0.3", "p", "v", 0.0, "losses.md:127"), ("L2EPSINS_0.3", "p", "v", 0.0, "losses.md:154"),
    ("L2EPSINS_0.3", "p", "d", 0.0, "losses.md:154"),
    ("MODHUBER", 1.0, "d", 0.0, "losses.md:397: a > 1 gives 0, and 2(a - 1) = 0 at a = 1"),
    ("MODHUBER", -1.0, "v", 4.0, "losses.md:397: a >= -1 takes the square"), ("MODHUBER", -1.0, "d", -4.0, "losses.md:397"),
    ("ZEROONE", 0.0, "v", 0.0, "losses.md:242: a >= 0 gives 0"), ("ZEROONE", -0.0, "v", 0.0, "losses.md:242: -0 < 0 is false"),
    ("PERCEPTRON", 0.0, "d", 0.0, "losses.md:268: a >= 0 gives slope 0"), ("PERCEPTRON", -0.0, "d", 0.0, "losses.md:268"),
    ("L1HINGE", 1.0, "d", 0.0, "losses.md:319: a >= 1 gives slope 0"), ("L2HINGE", 1.0, "d", 0.0, "losses.md:346"),
    ("SMOOTHEDL1HINGE_0.5", 0.5, "d", -1.0, "losses.md:371: a >= 1 - gamma takes (a - 1)/gamma = -1"),
    ("SMOOTHEDL1HINGE_2.0", -1.0, "d", -1.0, "losses.md:371"),
    ("DWDMARGIN_1.0", 0.5, "d", -1.0, "losses.md:503: a >= q/(q+1) takes 1 - a"), ("DWDMARGIN_1.0", 0.5, "v", 0.5, "losses.md:503"),
    ("DWDMARGIN_3.0", 0.75, "d", -1.0, "losses.md:503"), ("DWDMARGIN_3.0", 0.75, "v", 0.25, "losses.md:503"),
    ("LP_0.5", 0.0, "d", "nan", "losses.md:28: P |r|^(P-1) sign(r) = 0.5 · Inf · 0"),
    ("LP_0.5", -0.0, "d", "nan", "losses.md:28"), ("LPINT_-2", -0.0, "d", "nan", "losses.md:28"),
    ("LP_0.5", 0.0, "v", 0.0, "losses.md:28"), ("LP_1.7", 0.0, "d", 0.0, "losses.md:28: 1.7 · 0 · 0"),
    ("LPINT_-2", 0.0, "v", "inf", "losses.md:28: (1/0)^2"), ("LPINT_-2", 0.0, "d", "nan", "losses.md:28: -2 · Inf · sign(0)"),
    ("LPINT_-2", -0.0, "v", "inf", "losses.md:28: |−0| = +0"),
    ("LPINT_2", 0.0, "d", 0.0, "losses.md:28"), ("LPINT_3", 0.0, "d", 0.0, "losses.md:28"),
    ("SIGMOID", 0.0, "v", 1.0, "losses.md:476; the value keeps an absolute 4 eps(T): 1 - tanh a saturates as a grows, "
                               "not where a search converges"),
]

# ---- form-limited points: the reference's stated form leaves T although the true value is in T ---
# rule(name, T, u, exp) -> (which, verdict) pairs; exp is mpmath's
def form_limited(mp, name, T, u):
    out = []
    fmax = mp.mpf(float(np.finfo(T).max))
    if name == "LOGITMARGIN":
        if mp.exp(-mp.mpf(u)) > fmax:
            out.append(("v", np.inf))   # log1p(exp(-a)), exp overflows
        if mp.exp(mp.mpf(u)) > fmax:
            out.append(("d", 0.0))      # -1 / (1 + exp(a)) = -1 / Inf
    if name == "DWDMARGIN" and u == 0:  # c / a^q, c > 0, q odd here: the zero's sign; -s^(q+1) / 0^(q+1), q + 1 even
        out += [("v", float(np.copysign(np.inf, u))), ("d", -np.inf)]
    return out


# ---- rounding ------------------------------------------------------------------------------------------

def ulp_of(t, T):
    """The spacing of T at |t| (the smallest subnormal below the normal range)."""
    fi = np.finfo(T)
    a = np.abs(np.asarray(t, dtype=np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.floor(np.log2(np.where((a > 0) & np.isfinite(a), a, 1.0)))
        e = np.maximum(e, fi.minexp)
        return np.ldexp(1.0, (e - fi.nmant).astype(np.int64))


def rn(mp, v, T):
    """RN_T(v) for an mpmath v, as a Python float (±Inf on overflow), by comparing the neighbours exactly."""
    fi = np.finfo(T)
    fmax = mp.mpf(float(fi.max))
    if abs(v) >= fmax + mp.mpf(float(ulp_of(float(fi.max), T))) / 2:
        return float(np.inf) if v > 0 else float(-np.inf)
    with np.errstate(over="ignore"):
        c = T(float(v)) if T is np.float64 else np.float32(float(v))
    if not np.isfinite(c):
        c = T(np.copysign(fi.max, float(c)))
    cands = [c, np.nextafter(c, T(np.inf)), np.nextafter(c, T(-np.inf))]
    cands = [x for x in cands if np.isfinite(x)]
    best = min(cands, key=lambda x: (abs(mp.mpf(float(x)) - v), int(np.abs(x).view(np.uint32 if T is np.float32 else np.uint64)) & 1))
    return float(best)


def split(mp, v):
    """(hi, lo): RN_Float64(v) and (v - hi) in Float64 ulps of hi."""
    hi = float(v)
    if not np.isfinite(hi):
        return hi, 0.0
    lo = float((v - mp.mpf(hi)) / mp.mpf(float(ulp_of(hi, np.float64))))
    return hi, (lo if abs(lo) <= 0.5 else 0.0)  # below the subnormals: hi = 0 is within the smallest ulp


def generate():
    import mpmath as mp

    mp.mp.dps = DPS
    value, deriv = definitions(mp)
    out = {}
    conv_rows, form_rows = [], []
    for cfg, name, p, kind, line in CONFIGS:
        pm = None if p is None else mp.mpf(p)  # the Float64 field as given
        for tn, T in TNAMES.items():
            u = grid(cfg, name, p, kind, T)
            n = len(u)
            assert 40 <= n <= 90, (cfg, tn, n)
            cols = {k: np.zeros(n) for k in ("v_hi", "v_lo", "d_hi", "d_lo", "v_rn", "d_rn", "v_du", "d_du", "v_dp", "d_dp")}
            cols.update(v_form=np.full(n, np.nan), d_form=np.full(n, np.nan), v_conv=np.full(n, NOT_CONV), d_conv=np.full(n, NOT_CONV))
            is_form = {"v": np.zeros(n, bool), "d": np.zeros(n, bool)}
            # the convention points of this configuration
            for ccfg, cu, which, want, why in CONVENTIONS:
                if ccfg != cfg:
                    continue
                cu = {"p": float(T(p)) if p is not None else None, "-p": -float(T(p)) if p is not None else None}.get(cu, cu)
                if isinstance(cu, float) and float(T(cu)) != cu:
                    continue  # not a point of this dtype
                at = [i for i in range(n) if u[i] == cu and np.signbit(u[i]) == np.signbit(cu)]
                if cu == "p" or not at:
                    raise AssertionError(f"convention point {cfg} {cu!r} is not on the {tn} grid")
                w = {"nan": np.nan, "inf": np.inf}.get(want, want)
                w = float(T(w))  # a verdict is a value of T (Quantile's tau rounded once)
                if ccfg.startswith(("L1EPSINS", "L2EPSINS")) and abs(cu) > p:
                    continue  # RN_T(eps) above eps: the point is past the kink in this dtype
                cols[f"{which}_conv"][at[0]] = w
                conv_rows.append((cfg, tn, cu, which, w, f"docs/src/{why}"))
            for i in range(n):
                um = mp.mpf(float(u[i]))
                for which, fn in (("v", value), ("d", deriv)):
                    t = fn(name, pm, um)
                    if t is None:  # no value by the definition: a convention or form-limited point must cover it
                        cols[f"{which}_hi"][i] = cols[f"{which}_rn"][i] = np.nan
                        continue
                    cols[f"{which}_hi"][i], cols[f"{which}_lo"][i] = split(mp, t)
                    cols[f"{which}_rn"][i] = rn(mp, t, T)
                    if name in TRANSCENDENTAL and u[i] != 0 and np.isfinite(cols[f"{which}_rn"][i]):  # an overflow is matched as ±Inf
                        h = mp.mpf(float(ulp_of(u[i], T))) / 2
                        cols[f"{which}_du"][i] = float(max(abs(fn(name, pm, um + h) - t), abs(fn(name, pm, um - h) - t)))
                        if name in ("LP", "PERIODIC"):
                            e = mp.mpf(2) ** -53 * (3 if name == "PERIODIC" else 1)
                            cols[f"{which}_dp"][i] = float(max(abs(fn(name, pm * (1 + e), um) - t), abs(fn(name, pm * (1 - e), um) - t)))
                for which, verdict in form_limited(mp, name, T, float(u[i])):
                    cols[f"{which}_form"][i] = verdict
                    is_form[which][i] = True
                    form_rows.append((cfg, tn, float(u[i]), which, verdict))
            for which in ("v", "d"):
                covered = is_form[which] | (cols[f"{which}_conv"] != NOT_CONV)
                ok = covered | ((np.isfinite(cols[f"{which}_hi"]) | np.isinf(cols[f"{which}_rn"])) & np.isfinite(cols[f"{which}_du"])
                                & np.isfinite(cols[f"{which}_dp"]) & ~np.isnan(cols[f"{which}_rn"]))
                assert ok.all(), (cfg, tn, which, u[~ok])
                assert is_form[which].sum() <= 0.10 * n, (cfg, tn, which, int(is_form[which].sum()), n)
                # a written verdict that the definition also gives must agree with it
                both = (cols[f"{which}_conv"] != NOT_CONV) & np.isfinite(cols[f"{which}_hi"]) & np.isfinite(cols[f"{which}_conv"])
                assert np.all(cols[f"{which}_conv"][both] == cols[f"{which}_rn"][both]), (cfg, tn, which, u[both])
            pre = f"{cfg}/{tn}"
            out[f"{pre}/u"] = u
            for k, v in cols.items():
                out[f"{pre}/{k}"] = v.astype(np.float32) if k.endswith("_lo") else v
    out["configs/name"] = np.array([c[0] for c in CONFIGS], dtype="U24")
    out["configs/loss"] = np.array([c[1] for c in CONFIGS], dtype="U24")
    out["configs/param"] = np.array([np.nan if c[2] is None else c[2] for c in CONFIGS])
    out["configs/kind"] = np.array([c[3] for c in CONFIGS], dtype="U8")
    out["configs/line"] = np.array([c[4] for c in CONFIGS], dtype=np.int32)
    for j, key in enumerate(("config", "T", "u", "which", "want", "line")):
        col = [r[j] for r in conv_rows]
        out[f"conv/{key}"] = np.array(col, dtype=np.float64 if key in ("u", "want") else "U160")
    for j, key in enumerate(("config", "T", "u", "which", "want")):
        col = [r[j] for r in form_rows]
        out[f"form/{key}"] = np.array(col, dtype=np.float64 if key in ("u", "want") else "U24")
    return out


def main():
    out = generate()
    path = Path(__file__).with_name("losses.npz")
    np.savez_compressed(path, **out)
    npts = sum(v.size for k, v in out.items() if k.endswith("/u") and not k.startswith(("conv", "form")))
    print("wrote", len(out), "arrays,", npts, "points,", len(out["conv/u"]), "conventions,", len(out["form/u"]),
          "form-limited,", path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
