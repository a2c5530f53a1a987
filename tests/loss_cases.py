"""Shared by tests/test_loss_values.py (CPU) and tests/test_loss_values_gpu.py: the loss fixture
(tests/golden/losses.npz, written by tests/golden/make_loss_golden.py from mpmath), the bounds, the comparison
of per-point results with it, and the layout of the one-hot datasets.

Bounds, written before the first GPU run and fitted to nothing the engine returns:
  algebraic losses   (L1, L2, LPINT, Huber, both ε-insensitive losses, Quantile, ZeroOne, Perceptron, the hinges,
                     ModHuber, L2Margin, SmoothedL1Hinge, DWDMargin, and their derivatives): 2 ulp_T(true). In
                     Float32 the parametric ones (a Float64 field) are evaluated in Float64 and rounded once:
                     1 ulp_T. No conditioning term: their arguments are exact.
  the others         (LP, LogCosh, LogitDist, LogitMargin, Exp, Periodic, Sigmoid's derivative): 4 ulp_T(true) per
                     transcendental value the stated form takes (the project's bar for a transcendental operator,
                     operator_cases.py), doubled where the value is squared, + 2 ulp where the form divides,
                     capped at 16 ulp_T (the derivative fixture's cap): ULPS below. In Float32 LP and Periodic
                     run in Float64 and are rounded once: 1 ulp_T. Every point also gets its conditioning: the
                     move of the true value under half an ulp_T of u and under the Float64 roundings of the
                     parameter (the fixture's *_du and *_dp).
  no allowance for cancellation, with one stated exception: Sigmoid's value 1 - tanh a keeps the absolute
                     4 eps(T) that test_margin_losses_gpu.py grants (it saturates as a grows, not where a search
                     converges);
  kinks, conventions and form-limited points: the written verdict, exactly (NaN matches NaN, ±Inf its sign);
  a true value beyond T's range is ±Inf (a finite result within the bound of floatmax passes too).
"""
import functools
import importlib.util
from pathlib import Path

import numpy as np

import srhip
from srhip import constants as K

GOLDEN = Path(__file__).resolve().parent / "golden"
NROWS = 549  # 512 + 37, as the operator tests
NFEAT = 16
PLANT_ROWS = (0, 63, 64, 130, 255, 256, 511, 512, 548)  # lanes, wave and tile borders, the partial tile
DTYPES = (np.float32, np.float64)
TNAME = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}

# ulps of T: (Float64, Float32) per loss and ("v", "d"). 4 per transcendental value, x2 when squared, +2 per division.
ULPS = {
    ("LP", "v"): (4, 1), ("LP", "d"): (6, 1),                   # pow; p · pow (one more product)
    # ln cosh: Float64 sinh squared, log1p; Float32 exp squared ((1 - q)²), log1p, a reciprocal. Derivative: tanh
    ("LOGCOSH", "v"): (12, 14), ("LOGCOSH", "d"): (4, 4),
    ("LOGITDIST", "v"): (12, 14), ("LOGITDIST", "d"): (4, 4),
    ("LOGITMARGIN", "v"): (8, 8), ("LOGITMARGIN", "d"): (6, 6),  # exp, log1p; exp and a division
    ("EXP", "v"): (4, 4), ("EXP", "d"): (4, 4),
    ("PERIODIC", "v"): (10, 1), ("PERIODIC", "d"): (6, 1),      # sin squared (2 sin²(x/2)); k · sin
    ("SIGMOID", "d"): (10, 10),                                # cosh squared, a division
}
PARAMETRIC_ALGEBRAIC = ("HUBER", "L1EPSINS", "L2EPSINS", "QUANTILE", "SMOOTHEDL1HINGE", "DWDMARGIN")
assert all(1 <= u <= 16 for v in ULPS.values() for u in v)


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location("make_loss_golden", GOLDEN / "make_loss_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def fixture():
    with np.load(GOLDEN / "losses.npz") as z:
        fx = {k: z[k] for k in z.files}
    for v in fx.values():
        v.setflags(write=False)
    return fx


def ulp_of(t, T):
    return generator().ulp_of(t, T)


def tname(T):
    return TNAME[np.dtype(T)]


@functools.lru_cache(maxsize=None)
def configs():
    """[(config, loss name, parameter or None, "dist" | "margin")]."""
    fx = fixture()
    return [(str(n), str(l), None if np.isnan(p) else float(p), str(k))
            for n, l, p, k in zip(fx["configs/name"], fx["configs/loss"], fx["configs/param"], fx["configs/kind"])]


def config(cfg):
    return next(c for c in configs() if c[0] == cfg)


def loss_of(cfg):
    """The srhip loss object of a configuration."""
    _, name, p, _ = config(cfg)
    if name == "LPINT":
        return srhip.LPDistLoss(int(p))
    return srhip.options.SupervisedLoss(K.LOSS[name], 0.0 if p is None else p)


@functools.lru_cache(maxsize=None)
def case(cfg, T):
    """The fixture's arrays of one configuration and dtype, by their short names (u, v_hi, ...)."""
    fx, pre = fixture(), f"{cfg}/{tname(T)}/"
    return {k[len(pre):]: v for k, v in fx.items() if k.startswith(pre)}


def n_ulps(cfg, T, which):
    _, name, p, _ = config(cfg)
    f32 = np.dtype(T) == np.float32
    if (name, which) in ULPS:
        return ULPS[(name, which)][1 if f32 else 0]
    assert name not in generator().TRANSCENDENTAL or (name, which) == ("SIGMOID", "v")
    return 1 if (f32 and name in PARAMETRIC_ALGEBRAIC) else 2


def verdict(c, which):
    """(want, fixed): per point the exactly matched verdict (convention, then form-limited) and whether it has one."""
    conv, form = c[f"{which}_conv"], c[f"{which}_form"]
    is_conv = conv != generator().NOT_CONV
    is_form = ~np.isnan(form) & ~is_conv
    return np.where(is_conv, conv, np.where(is_form, form, np.nan)), is_conv | is_form


def bound(cfg, T, which, idx=None):
    """The absolute bound per point (the points with a verdict and the overflowing ones are matched, not bounded)."""
    c = case(cfg, T)
    idx = np.arange(len(c["u"])) if idx is None else idx
    _, name, _, _ = config(cfg)
    hi = c[f"{which}_hi"][idx]
    if (name, which) == ("SIGMOID", "v"):
        return np.full(len(idx), 4 * float(np.finfo(T).eps))
    return n_ulps(cfg, T, which) * ulp_of(np.where(np.isfinite(hi), hi, 1.0), T) + c[f"{which}_du"][idx] + c[f"{which}_dp"][idx]


def same(got, want):
    """Equal as values of T: NaN matches NaN, an infinity its sign, a zero either zero (a sum cannot show the sign)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return (got == want) | (np.isnan(got) & np.isnan(want))


def ratio(got, cfg, T, which, idx=None):
    """err / bound per point of `idx` (0 where a verdict or an overflow is matched, Inf where it is not)."""
    c = case(cfg, T)
    idx = np.arange(len(c["u"])) if idx is None else np.asarray(idx)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == idx.shape, (got.shape, idx.shape)
    want, fixed = verdict(c, which)
    want, fixed = want[idx], fixed[idx]
    hi, lo, rn = c[f"{which}_hi"][idx], c[f"{which}_lo"][idx].astype(np.float64), c[f"{which}_rn"][idx]
    b = bound(cfg, T, which, idx)
    with np.errstate(all="ignore"):
        err = np.abs((got - hi) - lo * ulp_of(hi, np.float64))
        r = np.where(np.isfinite(got) & np.isfinite(hi), err / b, np.inf)
        # the true value leaves T: ±Inf, or a finite result within the bound of the true value
        over = np.isinf(rn)
        r = np.where(over & (got == rn), 0.0, r)
    return np.where(fixed, np.where(same(got, want), 0.0, np.inf), r)


def check(got, cfg, T, which, what, idx=None):
    """Every point within its bound; returns the worst err / bound."""
    c = case(cfg, T)
    idx = np.arange(len(c["u"])) if idx is None else np.asarray(idx)
    r = ratio(got, cfg, T, which, idx)
    if not np.all(r <= 1.0):
        bad = np.flatnonzero(~(r <= 1.0))
        want, fixed = verdict(c, which)
        rows = [(float(c["u"][idx[i]]), float(np.asarray(got)[i]), float(want[idx[i]] if fixed[idx[i]] else c[f"{which}_hi"][idx[i]]),
                 float(r[i])) for i in bad[:6]]
        raise AssertionError(f"{what} {cfg} {tname(T)} {'value' if which == 'v' else 'derivative'}: {len(bad)} of {len(r)} points "
                             f"beyond the bound; (u, got, true, err/bound): {rows}")
    return float(np.max(r)) if len(r) else 0.0


# ---- the one-hot datasets ---------------------------------------------------------------------------------

def fill_points(cfg, T, derivative=False):
    """Indices of the points a fill row may hold: finite ℓ (and ℓ' for the gradient datasets) by the fixture and
    by every verdict, so that 0 · ℓ is 0."""
    c = case(cfg, T)
    ok = np.ones(len(c["u"]), bool)
    for which in ("v", "d") if derivative else ("v",):
        want, fixed = verdict(c, which)
        ok &= np.where(fixed, np.isfinite(want), np.isfinite(c[f"{which}_rn"]))
        # away from T's edge: another form of the same loss may round an almost-overflowing value to Inf
        ok &= np.abs(np.where(np.isfinite(c[f"{which}_hi"]), c[f"{which}_hi"], np.inf)) < 1e30
    assert ok.sum() >= 20, (cfg, tname(T), int(ok.sum()))
    return np.flatnonzero(ok)


def hot_points(cfg, T, derivative=False):
    """The points a launch can make hot: all of them; the gradient trees c0 + x turn -0 into +0, so -0 is left out."""
    u = case(cfg, T)["u"]
    return np.flatnonzero(~((u == 0) & np.signbit(u))) if derivative else np.arange(len(u))


def in_routine_range(cfg, T):
    """Per point: inside the Float32 Periodic routines' Cody-Waite range |r·k| <= kCwCosMax (every point of another
    loss). The points beyond it go in datasets of their own: a row there hands the tree back to the interpreter."""
    c = case(cfg, T)
    _, name, p, _ = config(cfg)
    if name != "PERIODIC":
        return np.ones(len(c["u"]), bool)
    return np.abs(c["u"]) * (2 * np.pi / p) <= generator().CW_COS_MAX


def launches(cfg, T, derivative=False, nrows=NROWS, first_row=0, beyond=False):
    """[(X (NFEAT + 1, nrows) Float64, hot row, the 16 hot points' indices)]: feature f cycles through the fill
    points from its own start, so neighbouring lanes take different branches, and holds its hot point in the hot
    row, which walks PLANT_ROWS; the last feature is the deep family's pad column. Every point is hot once.
    `beyond`: the launches whose hot points lie beyond the Periodic routines' range (the fill never does)."""
    c = case(cfg, T)
    inside = in_routine_range(cfg, T)
    fill, hot = fill_points(cfg, T, derivative), hot_points(cfg, T, derivative)
    fill, hot = fill[inside[fill]], hot[inside[hot] != beyond]
    pad = np.random.default_rng(0).uniform(0.5, 1.5, nrows).astype(np.float32).astype(np.float64)
    out = []
    for j, h0 in enumerate(range(0, len(hot), NFEAT)):
        pts = hot[(h0 + np.arange(NFEAT)) % len(hot)]
        rho = PLANT_ROWS[(first_row + j) % len(PLANT_ROWS)] % nrows
        X = np.empty((NFEAT + 1, nrows))
        for f in range(NFEAT):
            X[f] = c["u"][fill[(np.arange(nrows) + 7 * f + 3 * j) % len(fill)]]
            X[f, rho] = c["u"][pts[f]]
        X[NFEAT] = pad
        out.append((X, rho, pts))
    return out
