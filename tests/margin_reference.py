"""NumPy restatement of LossFunctions.jl's margin losses on the agreement
a = y·ŷ (docs/src/losses.md:226-520 of the reference; the derivatives are the
ones LossFunctions.jl defines), written from the table of include/srhip.h and
independent of the engine's device code. The checker of
tests/test_margin_losses*.py: applied to the oracle's per-row predictions.

The nine losses without a parameter are evaluated on arrays of the dtype T of
`a`; SmoothedL1Hinge(γ) and DWDMargin(q) hold a Float64 field, so they are
evaluated in float64 on the T-valued `a` and rounded to T once.
"""
import numpy as np

from srhip import constants as K

L = K.LOSS
PARAMETRIC = (L["SMOOTHEDL1HINGE"], L["DWDMARGIN"])
NAMES = ["ZEROONE", "PERCEPTRON", "LOGITMARGIN", "L1HINGE", "L2HINGE", "SMOOTHEDL1HINGE", "MODHUBER", "L2MARGIN",
         "EXP", "SIGMOID", "DWDMARGIN"]


def _value(kind, p, a):
    """L(a) in the dtype of a (p a Python float)."""
    T = a.dtype.type
    one, zero = T(1), T(0)
    h = np.maximum(zero, one - a)
    if kind == L["ZEROONE"]:
        return np.where(a < zero, one, zero)
    if kind == L["PERCEPTRON"]:
        return np.maximum(zero, -a)
    if kind == L["LOGITMARGIN"]:
        return np.log1p(np.exp(-a))
    if kind == L["L1HINGE"]:
        return h
    if kind == L["L2HINGE"]:
        return h * h
    if kind == L["SMOOTHEDL1HINGE"]:
        return np.where(a >= one - T(p), T(0.5 / p) * (h * h), one - T(p / 2) - a)
    if kind == L["MODHUBER"]:
        return np.where(a >= -one, h * h, T(-4) * a)
    if kind == L["L2MARGIN"]:
        return (one - a) * (one - a)
    if kind == L["EXP"]:
        return np.exp(-a)
    if kind == L["SIGMOID"]:
        return one - np.tanh(a)
    assert kind == L["DWDMARGIN"]
    return np.where(a >= T(p / (p + 1)), one - a, T(p ** p / (p + 1) ** (p + 1)) / a ** T(p))


def _deriv(kind, p, a):
    """L'(a) in the dtype of a."""
    T = a.dtype.type
    one, zero = T(1), T(0)
    if kind == L["ZEROONE"]:
        return np.zeros_like(a)
    if kind == L["PERCEPTRON"]:
        return np.where(a >= zero, zero, -one)
    if kind == L["LOGITMARGIN"]:
        return -one / (one + np.exp(a))
    if kind == L["L1HINGE"]:
        return np.where(a >= one, zero, -one)
    if kind == L["L2HINGE"]:
        return np.where(a >= one, zero, T(2) * (a - one))
    if kind == L["SMOOTHEDL1HINGE"]:
        return np.where(a >= one - T(p), np.where(a >= one, zero, (a - one) / T(p)), -one)
    if kind == L["MODHUBER"]:
        return np.where(a >= -one, np.where(a > one, zero, T(2) * (a - one)), T(-4))
    if kind == L["L2MARGIN"]:
        return T(2) * (a - one)
    if kind == L["EXP"]:
        return -np.exp(-a)
    if kind == L["SIGMOID"]:
        c = np.cosh(a)
        return -one / (c * c)  # -sech(a)^2
    assert kind == L["DWDMARGIN"]
    s = p / (p + 1)
    return np.where(a >= T(s), -one, T(-(s ** (p + 1))) / a ** T(p + 1))


def _apply(f, kind, param, a):
    a = np.asarray(a)
    T = a.dtype
    assert T in (np.float32, np.float64)
    with np.errstate(all="ignore"):
        if kind in PARAMETRIC:
            return f(kind, float(param), a.astype(np.float64)).astype(T)
        return f(kind, float(param), a).astype(T)


def value(kind, param, a):
    """Elementwise L(a), in the dtype of `a`."""
    return _apply(_value, kind, param, a)


def deriv(kind, param, a):
    """Elementwise L'(a), in the dtype of `a` (the gradient seed is dℓ/dŷ = y·L'(y·ŷ))."""
    return _apply(_deriv, kind, param, a)
