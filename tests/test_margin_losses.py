"""Margin (classification) losses, the parts that need no GPU: the ids of
include/srhip.h against the Python mirror and the constructors, the Julia
binding's constants and loss_code methods (a static text check, as
tests/test_julia_binding.py), and the Float32 loss tree code built without a
device: it compiles for every margin id and ends its tile with the agreement
ŷ·y (a multiply) where a distance loss has the residual ŷ - y (a subtract);
gradient and Float64 tree code answer UNSUPPORTED (they run interpreted)."""
import re
from pathlib import Path

import numpy as np
import pytest

import margin_reference as M
import srhip
from srhip import constants as K

ROOT = Path(__file__).resolve().parent.parent
HDR = (ROOT / "include" / "srhip.h").read_text()
JL = (ROOT / "symbolicregression.jl_amd" / "julia" / "SRHip.jl").read_text()

# constructor, header name, parameter the constructor is given here
CTORS = [
    (srhip.ZeroOneLoss, "ZEROONE", None), (srhip.PerceptronLoss, "PERCEPTRON", None),
    (srhip.LogitMarginLoss, "LOGITMARGIN", None), (srhip.L1HingeLoss, "L1HINGE", None),
    (srhip.L2HingeLoss, "L2HINGE", None), (srhip.SmoothedL1HingeLoss, "SMOOTHEDL1HINGE", 0.5),
    (srhip.ModifiedHuberLoss, "MODHUBER", None), (srhip.L2MarginLoss, "L2MARGIN", None),
    (srhip.ExpLoss, "EXP", None), (srhip.SigmoidLoss, "SIGMOID", None), (srhip.DWDMarginLoss, "DWDMARGIN", 1.0),
]
# LossFunctions type, header name, the field loss_code reads
JULIA = [("ZeroOneLoss", "ZEROONE", None), ("PerceptronLoss", "PERCEPTRON", None),
         ("LogitMarginLoss", "LOGITMARGIN", None), ("L1HingeLoss", "L1HINGE", None), ("L2HingeLoss", "L2HINGE", None),
         ("SmoothedL1HingeLoss", "SMOOTHEDL1HINGE", "gamma"), ("ModifiedHuberLoss", "MODHUBER", None),
         ("L2MarginLoss", "L2MARGIN", None), ("ExpLoss", "EXP", None), ("SigmoidLoss", "SIGMOID", None),
         ("DWDMarginLoss", "DWDMARGIN", "q")]


def header_losses():
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define SRHIP_LOSS_(\w+)\s+(\d+)", HDR)}


def margin_losses():
    return [c() if p is None else c(p) for c, _, p in CTORS]


def test_header_ids_constants_and_constructors():
    hdr = header_losses()
    assert hdr == K.LOSS
    assert int(re.search(r"#define SRHIP_NUM_LOSSES (\d+)", HDR).group(1)) == len(K.LOSSES) == 22
    begin = int(re.search(r"#define SRHIP_MARGIN_LOSS_BEGIN (\d+)", HDR).group(1))
    assert begin == K.MARGIN_LOSS_BEGIN == 11
    assert [hdr[n] for n in M.NAMES] == list(range(11, 22))  # appended after LPINT, in the issue's order
    assert hdr["LPINT"] == 10 and hdr["L2"] == 0  # the distance ids stay
    for ctor, name, p in CTORS:
        loss = ctor() if p is None else ctor(p)
        assert isinstance(loss, srhip.SupervisedLoss)
        assert loss.kind == hdr[name], name
        assert loss.params == [0.0 if p is None else p], name
    assert srhip.HingeLoss is srhip.L1HingeLoss
    assert srhip.Options(binary_operators=["+"], elementwise_loss=srhip.SigmoidLoss()).elementwise_loss.kind == 20


def test_julia_binding_maps_every_margin_loss():
    hdr = header_losses()
    consts = {}
    for lhs, rhs in re.findall(r"const ((?:LOSS_\w+,?\s*)+)=\s*((?:Int32\(\d+\),?\s*)+)", JL):
        names = [x.strip() for x in lhs.split(",") if x.strip()]
        consts.update(zip(names, [int(v) for v in re.findall(r"Int32\((\d+)\)", rhs)]))
    using = re.search(r"using LossFunctions:(.*?)\nimport", JL, re.S).group(1)
    for typ, name, field in JULIA:
        assert consts.get(f"LOSS_{name}") == hdr[name], name
        assert re.search(rf"\b{typ}\b", using), f"{typ} is not imported from LossFunctions"
        arg = rf"l::{typ}" if field else rf"::{typ}"
        par = rf"Float64\(l\.{field}\)" if field else r"0\.0"
        assert re.search(rf"^loss_code\({arg}\) = \(LOSS_{name}, {par}\)$", JL, re.M), typ


def _flat(T=np.float32):
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=[])
    trees = srhip.random_population(24, o, 5, T, seed=5)
    return srhip.flatten(trees, o, dtype=T)


@pytest.mark.parametrize("fast", [0, 1])
def test_loss_tree_code_compiles_with_the_agreement_in_the_tail(fast):
    flat = _flat()
    def instructions(text):  # without the alignment padding between trees and the offset comments
        return [l for l in text.splitlines() if l != "s_nop 0" and not l.startswith("; tree code at")]

    _, ref_text, ref_offs = srhip.engine.jit_compile(flat, fast=bool(fast), loss=srhip.L1DistLoss())
    ref_lines = instructions(ref_text)
    for loss in margin_losses():
        code, text, offs = srhip.engine.jit_compile(flat, fast=bool(fast), loss=loss)
        assert len(code) > 0 and sorted(offs) == sorted(ref_offs), loss.kind
        lines = instructions(text)
        assert len(lines) == len(ref_lines), loss.kind
        diff = [(a, b) for a, b in zip(ref_lines, lines) if a != b]
        # the same code but for the tile tail: ŷ·y where L1 has ŷ - y (the packed subtract is
        # v_pk_add_f32 with the second operand negated), and the routine's address and parameter
        subs = [(a, b) for a, b in diff if a.startswith(("v_sub_f32_e32", "v_pk_add_f32"))]
        assert subs, loss.kind
        for a, b in subs:
            assert b.startswith("v_mul_f32_e32" if a.startswith("v_sub") else "v_pk_mul_f32"), (a, b)
            assert "neg" not in b
        # one tail per tree: 4 scalar or 2 packed instructions
        assert len(subs) in (4 * len(offs), 2 * len(offs)), (loss.kind, len(subs), len(offs))
        others = [(a, b) for a, b in diff if (a, b) not in subs]
        # (a parameter that is no inline constant takes a literal: the branches over it move)
        assert all(a.split()[0] == b.split()[0] and
                   (a.split()[0] in ("s_add_u32", "s_addc_u32", "s_mov_b32") or a.startswith(("s_cbranch", "s_branch")))
                   for a, b in others), others[:4]


def test_gradient_and_float64_tree_code_are_unsupported():
    flat32, flat64 = _flat(), _flat(np.float64)
    for loss in margin_losses():
        with pytest.raises(srhip.Unsupported):
            srhip.engine.jit_compile(flat32, grad=True, loss=loss)  # grad = 1
        with pytest.raises(srhip.Unsupported):
            srhip.engine.jit_compile(flat64, loss=loss)  # fast bit 3: the Float64 tree compiler
        with pytest.raises(srhip.Unsupported):
            srhip.engine.jit_compile(flat64, grad=True, loss=loss)
    # the distance losses keep theirs
    assert srhip.engine.jit_compile(flat32, grad=True, loss=srhip.L1DistLoss())[0]
    assert srhip.engine.jit_compile(flat64, loss=srhip.L1DistLoss())[0]


def test_reference_values_at_the_kinks():
    """The checker itself: hand-computed values of the table at and around every kink."""
    a = np.array([-2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 3.0])
    L = K.LOSS
    assert M.value(L["ZEROONE"], 0, a).tolist() == [1, 1, 0, 0, 0, 0, 0]
    assert M.value(L["PERCEPTRON"], 0, a).tolist() == [2, 1, 0, 0, 0, 0, 0]
    assert M.value(L["L1HINGE"], 0, a).tolist() == [3, 2, 1, 1, 0.5, 0, 0]
    assert M.value(L["L2HINGE"], 0, a).tolist() == [9, 4, 1, 1, 0.25, 0, 0]
    assert M.value(L["MODHUBER"], 0, a).tolist() == [8, 4, 1, 1, 0.25, 0, 0]
    assert M.value(L["L2MARGIN"], 0, a).tolist() == [9, 4, 1, 1, 0.25, 0, 4]
    assert M.value(L["SMOOTHEDL1HINGE"], 0.5, a).tolist() == [2.75, 1.75, 0.75, 0.75, 0.25, 0, 0]
    assert M.value(L["DWDMARGIN"], 1.0, a)[[0, 1, 4, 5, 6]].tolist() == [-0.125, -0.25, 0.5, 0, -2]
    assert np.allclose(M.value(L["LOGITMARGIN"], 0, a), np.log(1 + np.exp(-a)))
    assert np.allclose(M.value(L["SIGMOID"], 0, a), 1 - np.tanh(a)) and np.allclose(M.value(L["EXP"], 0, a), np.exp(-a))
    assert M.deriv(L["PERCEPTRON"], 0, a).tolist() == [-1, -1, 0, 0, 0, 0, 0]
    assert M.deriv(L["L1HINGE"], 0, a).tolist() == [-1, -1, -1, -1, -1, 0, 0]
    assert M.deriv(L["L2HINGE"], 0, a).tolist() == [-6, -4, -2, -2, -1, 0, 0]
    assert M.deriv(L["MODHUBER"], 0, a).tolist() == [-4, -4, -2, -2, -1, 0, 0]
    assert M.deriv(L["SMOOTHEDL1HINGE"], 0.5, a).tolist() == [-1, -1, -1, -1, -1, 0, 0]
    assert M.deriv(L["DWDMARGIN"], 1.0, a)[[0, 1, 4, 5, 6]].tolist() == [-0.0625, -0.25, -1, -1, -1]
    assert not M.deriv(L["ZEROONE"], 0, a).any()
    # the derivatives of the smooth ones against a central difference
    x = np.linspace(-3, 3, 13)
    for name in ("LOGITMARGIN", "EXP", "SIGMOID", "L2MARGIN"):
        fd = (M.value(L[name], 0, x + 1e-6) - M.value(L[name], 0, x - 1e-6)) / 2e-6
        assert np.allclose(M.deriv(L[name], 0, x), fd, rtol=1e-6, atol=1e-8), name
    # Float32 input: the values stay Float32 (the parametric ones rounded once from Float64)
    a32 = a.astype(np.float32)
    for name in M.NAMES:
        assert M.value(L[name], 0.5 if name == "SMOOTHEDL1HINGE" else 1.0, a32).dtype == np.float32
