"""Every elementwise loss's per-row value and derivative against the independent fixture tests/golden/losses.npz
(mpmath at 80 digits from the mathematical definitions; tests/golden/make_loss_golden.py), on the CPU.

The engine is held to the same fixture in every kernel family by tests/test_loss_values_gpu.py. This file keeps
the fixture honest (it loads, holds the edges it exists for, every point has a finite bound, it is what its
generator says), pins the three CPU references the other loss tests compare with — the oracle's elem_loss,
tests/margin_reference.py and test_jit_losses_gpu._dloss — to it with the bounds of loss_cases.py, and states,
from a NumPy emulation with T arithmetic per step, which written forms of a loss cannot meet those bounds.
"""
import numpy as np
import pytest

import loss_cases as C
import margin_reference as M
import oracle
from srhip import constants as K

TIDS = dict(ids=lambda T: np.dtype(T).name)
DIST = [c[0] for c in C.configs() if c[3] == "dist"]
MARGIN = [c[0] for c in C.configs() if c[3] == "margin"]


def test_the_fixture_covers_every_loss():
    assert len(DIST) == 15 and len(MARGIN) == 13
    assert {c[1] for c in C.configs()} == set(K.LOSS), set(K.LOSS) - {c[1] for c in C.configs()}
    assert {c[0] for c in C.configs() if c[1] == "LPINT"} == {"LPINT_2", "LPINT_3", "LPINT_4", "LPINT_-2"}
    gen = C.generator()
    assert gen.DPS >= 60
    npts = 0
    for cfg, name, p, kind in C.configs():
        for T in C.DTYPES:
            c = C.case(cfg, T)
            u = c["u"]
            assert 40 <= len(u) <= 90, (cfg, len(u))
            assert np.array_equal(u.astype(T).astype(np.float64), u)  # arguments exact in T
            assert np.array_equal(np.sort(u[u > 0]), np.sort(-u[u < 0]))  # both signs
            assert np.sum((u == 0) & np.signbit(u)) == 1 and np.sum((u == 0) & ~np.signbit(u)) == 1
            for which in ("v", "d"):
                want, fixed = C.verdict(c, which)
                form = ~np.isnan(c[f"{which}_form"])
                assert form.sum() <= 0.10 * len(u), (cfg, which)
                b = C.bound(cfg, T, which)
                free = ~fixed & ~np.isinf(c[f"{which}_rn"])
                assert np.isfinite(b[free]).all() and (b[free] > 0).all() and np.isfinite(c[f"{which}_hi"][free]).all(), (cfg, which)
            assert len(C.fill_points(cfg, T, True)) >= 20
            npts += len(u)
    assert npts > 3000
    fx = C.fixture()
    assert len(fx["conv/u"]) >= 50 and all(str(l).startswith("docs/src/losses.md:") for l in fx["conv/line"])
    assert (C.GOLDEN / "losses.npz").stat().st_size < 400_000  # of the order of the other two fixtures


def test_the_grids_hold_the_edges():
    f32, f64 = np.float32, np.float64
    for T, kmin in ((f32, 24), (f64, 50)):
        fi = np.finfo(T)
        for cfg in DIST + MARGIN:
            u = set(C.case(cfg, T)["u"])
            assert {float(fi.smallest_subnormal), float(fi.tiny), 2.0 ** -kmin, 2.0 ** -12, 1.0, 10.0, 44.0, 88.0, 89.0, 160.0, 161.0,
                    709.0, 710.0, 1e4} <= u, cfg
            assert {-88.0, -89.0, -709.0, -710.0} <= u
        s = T(np.sqrt(f64(fi.max)))
        for cfg in ("L2", "LPINT_2", "LPINT_4", "LPINT_-2"):
            assert {float(np.nextafter(s, T(0))), float(s), float(np.nextafter(s, T(np.inf)))} <= set(C.case(cfg, T)["u"])
        c = C.case("L2", T)
        assert np.isinf(c["v_rn"]).any() and np.isfinite(c["v_rn"][np.abs(c["u"]) > 1e15]).any()  # both sides of the overflow
        for cfg, kink in (("HUBER_0.8", 0.8), ("L1EPSINS_0.3", 0.3), ("L2EPSINS_0.3", 0.3), ("SMOOTHEDL1HINGE_0.5", 0.5),
                          ("DWDMARGIN_1.0", 0.5), ("DWDMARGIN_3.0", 0.75), ("L1HINGE", 1.0), ("MODHUBER", 1.0)):
            u = C.case(cfg, T)["u"]
            k = T(kink)
            near = [k] if kink == 1.0 else [k]
            lo, hi = k, k
            for _ in range(2):
                lo, hi = np.nextafter(lo, T(-np.inf)), np.nextafter(hi, T(np.inf))
                near += [lo, hi]
            assert {float(v) for v in near} - ({1.0} if kink == 1.0 else set()) <= set(u), (cfg, T)
        assert -1.0 in C.case("MODHUBER", T)["u"] and -1.0 in C.case("SMOOTHEDL1HINGE_2.0", T)["u"]
        u = C.case("PERIODIC_2.0", T)["u"]
        assert {0.5, 1.0, 1.5, 2.0, 3.0, 509295.0, 509297.0, 1e7} <= set(u)
        assert 509295.0 * np.pi < C.generator().CW_COS_MAX < 509297.0 * np.pi
    # the form-limited table: Float32 LogitMargin below a = -88.7 (as test_margin_losses_gpu.py states), DWDMargin at 0
    fx = C.fixture()
    forms = {(str(c), str(t), float(u), str(w)) for c, t, u, w in zip(fx["form/config"], fx["form/T"], fx["form/u"], fx["form/which"])}
    assert ("LOGITMARGIN", "f32", -89.0, "v") in forms and ("LOGITMARGIN", "f32", -88.0, "v") not in forms
    assert ("LOGITMARGIN", "f64", -710.0, "v") in forms and ("LOGITMARGIN", "f64", -709.0, "v") not in forms
    assert ("DWDMARGIN_1.0", "f32", 0.0, "v") in forms and ("DWDMARGIN_3.0", "f64", 0.0, "d") in forms


def test_fixture_regenerates_bit_for_bit():
    """With mpmath at hand: the generator's arrays equal the committed ones bit for bit."""
    pytest.importorskip("mpmath")
    out, fx = C.generator().generate(), C.fixture()
    assert set(out) == set(fx)
    for k, v in out.items():
        assert v.dtype == fx[k].dtype and v.tobytes() == fx[k].tobytes(), k


# ---- the CPU references of the other loss tests ------------------------------------------------------------

@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("cfg", DIST)
def test_oracle_elem_loss(cfg, T):
    """oracle.elem_loss (sr_oracle_eval.h) at every point, with the residual as ŷ - 0 and as 0 - (-r)."""
    c, loss = C.case(cfg, T), C.loss_of(cfg)
    with np.errstate(all="ignore"):
        got = np.array([oracle.elem_loss(loss.kind, loss.params, T(u), T(0), dtype=T) for u in c["u"]], dtype=np.float64)
        neg = np.array([oracle.elem_loss(loss.kind, loss.params, T(0), T(-u), dtype=T) for u in c["u"]], dtype=np.float64)
    C.check(got, cfg, T, "v", "oracle.elem_loss")
    keep = np.flatnonzero(~((c["u"] == 0) & np.signbit(c["u"])))  # 0 - (+0) is +0
    C.check(neg[keep], cfg, T, "v", "oracle.elem_loss (y = -r)", keep)


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("cfg", MARGIN)
def test_margin_reference(cfg, T):
    c, loss = C.case(cfg, T), C.loss_of(cfg)
    a = c["u"].astype(T)
    C.check(M.value(loss.kind, loss.param, a), cfg, T, "v", "margin_reference.value")
    C.check(M.deriv(loss.kind, loss.param, a), cfg, T, "d", "margin_reference.deriv")


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("cfg", [c for c in DIST if c != "L2" and not c.startswith("LPINT")])
def test_dloss_of_the_tree_code_loss_tests(cfg, T):
    """test_jit_losses_gpu._dloss, the seed reference of the gradient tree code's loss tests: Float64 of the T
    residual, held to the fixture after one rounding to T."""
    from test_jit_losses_gpu import _dloss

    c = C.case(cfg, T)
    with np.errstate(all="ignore"):
        got = np.asarray(_dloss(C.loss_of(cfg), c["u"]), dtype=np.float64).astype(T)
    C.check(got, cfg, T, "d", "_dloss")


# ---- which written forms can meet the bounds: a NumPy emulation, T arithmetic per step ------------------------
# libm here, not OCML, but the rounding grain a form cancels to is the same. The list below is what the GPU tests
# are expected to find in an engine that uses the form; it is written from this emulation, not from engine output.

LN2, LN4 = 0.69314718055994530942, 1.38629436111989061883


def three_term_logcosh(T, u):
    ar = np.abs(u).astype(T)
    return ar + np.log1p(np.exp(T(-2) * ar)) - T(LN2)


def three_term_logitdist(T, u):
    ar = np.abs(u).astype(T)
    return ar + T(2) * np.log1p(np.exp(-ar)) - T(LN4)


def lncosh_series_f32(h):
    """device_ops.h lncosh_f32, step by step in Float32 (a division for v_rcp_f32)."""
    f = np.float32
    q = np.exp(-h)
    s = f(1.0 / 5040.0)
    for k in (-1.0 / 720.0, 1.0 / 120.0, -1.0 / 24.0, 1.0 / 6.0, -0.5, 1.0):
        s = s * h + f(k)
    d = np.where(h < f(0.5), s * h, f(1) - q)
    return np.log1p(d * d * (f(0.5) * (f(1) / q)))


def lncosh_sinh(T, h):
    s = np.sinh(T(0.5) * h)
    return np.log1p(T(2) * s * s)


def stable_logcosh(T, u):
    ar = np.abs(u).astype(T)
    am = np.minimum(ar, T(80 if T is np.float32 else 700))
    return (lncosh_series_f32(am) if T is np.float32 else lncosh_sinh(T, am)) + (ar - am)


def stable_logitdist(T, u):
    ar = np.abs(u).astype(T)
    am = np.minimum(ar, T(160 if T is np.float32 else 1400))
    return T(2) * (lncosh_series_f32(T(0.5) * am) if T is np.float32 else lncosh_sinh(T, T(0.5) * am)) + (ar - am)


def one_minus_cos(T, u):
    """1 - cos(r·k) in Float64 (Float32 data: rounded once), k = 2π/c."""
    return (1.0 - np.cos(u * (6.28318530717958647692 / 2.0))).astype(T)


def two_sin_squared(T, u):
    s = np.sin(0.5 * (u * (6.28318530717958647692 / 2.0)))
    return (2.0 * s * s).astype(T)


FORMS = {  # label: (config, form)
    "LogCosh |r| + log1p(exp(-2|r|)) - ln 2": ("LOGCOSH", three_term_logcosh),
    "LogitDist |r| + 2 log1p(exp(-|r|)) - ln 4": ("LOGITDIST", three_term_logitdist),
    "Periodic 1 - cos(kr)": ("PERIODIC_2.0", one_minus_cos),
    "LogCosh log1p((1 - q)^2 / 2q) / log1p(2 sinh^2(h/2))": ("LOGCOSH", stable_logcosh),
    "LogitDist 2 ln cosh(r/2), the same": ("LOGITDIST", stable_logitdist),
    "Periodic 2 sin^2(kr/2)": ("PERIODIC_2.0", two_sin_squared),
}
# the forms that cannot meet the bounds, per dtype: the three-term forms and 1 - cos in both
BEYOND = {(label, T) for label in list(FORMS)[:3] for T in C.DTYPES}


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("label", list(FORMS))
def test_which_forms_meet_the_bounds(label, T):
    cfg, form = FORMS[label]
    c = C.case(cfg, T)
    with np.errstate(all="ignore"):
        got = np.asarray(form(T, c["u"]), dtype=np.float64)
    r = C.ratio(got, cfg, T, "v")
    worst = int(np.argmax(r))
    print(f"{label} {np.dtype(T).name}: worst err/bound {r[worst]:.3g} at u = {c['u'][worst]!r}; beyond at |u| in "
          f"{sorted(set(np.abs(c['u'][~(r <= 1)])))[:12]}")
    assert (not np.all(r <= 1.0)) == ((label, T) in BEYOND), (label, T, float(r[worst]), float(c["u"][worst]))
    if (label, T) in BEYOND:  # the converged regime is where it fails: every failing point has |u| k < 1
        k = np.pi if cfg.startswith("PERIODIC") else 1.0
        small = np.abs(c["u"]) * k < 0.1
        far = ~(r <= 1.0) & ~(np.abs(c["u"]) * k < 1.0)
        # 1 - cos also fails next to the zeros of the loss at multiples of c, for the same reason
        assert not far.any() or cfg.startswith("PERIODIC"), (label, c["u"][far])
        assert (~(r <= 1.0) & small).sum() >= 6
