"""The gradient tree code of expression losses without a GPU (SRHIP_LOSS_EXPR_GRAD_TREE_CODE, DESIGN.md
§3.12.2): the flag, the bindings, and the generator's bytes against llvm-mc's assembly of its own text."""
import re

import numpy as np
import pytest

import expr_loss_cases as E
import srhip
from srhip import Node, _lib
from srhip import constants as K
from srhip.engine import jit_compile
from test_expr_loss_tree_code import create_ex
from test_jit import LLVM, assemble, trans_forwarding_hazards
from test_julia_binding import JL


def d2(o):
    """(p - t) · (p + t): the prediction twice, exactly rounded operators"""
    return o.make_binary("*", o.make_binary("-", Node("x1"), Node("x2")), o.make_binary("+", Node("x1"), Node("x2")))


def explog(o):
    """exp(log(p / t)): log's NaN (p / t < 0) goes into a routine that marks its input"""
    return o.make_unary("exp", o.make_unary("log", o.make_binary("/", Node("x1"), Node("x2"))))


def folded(o):
    """(2 + 3) · (p - t): an operator on constants alone"""
    return o.make_binary("*", o.make_binary("+", Node(val=2.0), Node(val=3.0)), o.make_binary("-", Node("x1"), Node("x2")))


EXPRS = dict(E.EXPRS, D2=d2, EXPLOG=explog, FOLDED=folded)
LOSS_OPS = dict(binary_operators=["+", "-", "*", "/", "^"], unary_operators=["abs", "square", "log1p", "tanh", "log", "exp"])


def grad_loss(name, flagged=True):
    o = srhip.Options(**LOSS_OPS)
    return srhip.ExprLoss(EXPRS[name](o), o, grad_tree_code=flagged)


def test_flag_validation():
    assert K.LOSS_EXPR_GRAD_TREE_CODE == 4
    rc4, h4 = create_ex(4)
    rc5, h5 = create_ex(5)
    assert rc4 == 0 and rc5 == 0 and h5 == h4 + 1
    for flags in (8, 6):  # refused before anything is registered: the next handle follows h5
        assert create_ex(flags) == (_lib.ERR_INVALID, -1), flags
    rc0, h0 = create_ex(0)
    assert rc0 == 0 and h0 == h5 + 1
    for h in (h4, h5, h0):
        assert _lib.lib().srhip_loss_expr_destroy(h) == 0
    both = srhip.ExprLoss(E.sq(E.loss_options()), E.loss_options(), tree_code=True, grad_tree_code=True)
    assert both.grad_tree_code and both.tree_code and not grad_loss("SQ", flagged=False).grad_tree_code
    src = JL.read_text()
    assert re.search(r"tree_code::Bool=false,\s*grad_tree_code::Bool=false\) where", src)
    assert re.search(r"^const SRHIP_LOSS_EXPR_GRAD_TREE_CODE = UInt32\(4\)", src, re.M)


def batch():
    return srhip.flatten(E.problem(np.float32, 64, ntrees=64)[1], E.problem(np.float32, 64, ntrees=64)[0], dtype=np.float32)


@pytest.mark.skipif(not (LLVM / "llvm-mc").exists(), reason="llvm-mc not installed")
@pytest.mark.parametrize("name", ["SQ", "WSQ", "E1", "E2", "E5", "D2"])
def test_machine_code_equals_llvm_mc(name):
    code, text, offs = jit_compile(batch(), grad=True, loss=grad_loss(name))
    assert len(offs) >= 60, f"only {len(offs)} of 64 trees compiled"
    assert assemble(text) == code
    assert not trans_forwarding_hazards(text)


@pytest.mark.parametrize("name,flagged", [("E3", True), ("E4", True), ("FOLDED", True), ("SQ", False)])
def test_hook_refuses(name, flagged):
    with pytest.raises(srhip.SrhipError) as ei:
        jit_compile(batch(), grad=True, loss=grad_loss(name, flagged))
    assert ei.value.code == _lib.ERR_UNSUPPORTED
