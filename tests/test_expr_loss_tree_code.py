"""The opt-in tree-code form of expression losses without a GPU (include/srhip.h "expression
losses", SRHIP_LOSS_EXPR_TREE_CODE): the flag's validation, the Python keyword, the prototype and
the Julia ccall against the header, and the host statement of the semantics, which the flag does
not touch. The GPU side is tests/test_expr_loss_tree_code_gpu.py."""
import ctypes as C
import re

import numpy as np
import pytest

import expr_loss_cases as E
import srhip
from srhip import _lib
from srhip import constants as K
from test_julia_binding import JL, _c_kind, _jl_kind, header_prototypes, julia_ccalls

SUB = K.BOP["SUB"]


def create_ex(flags):
    """(rc, handle) of srhip_loss_expr_create_ex on the stream of p - t."""
    kind = np.array([K.NODE_FEATURE, K.NODE_FEATURE, K.NODE_BINARY], dtype=np.uint8)
    arg = np.array([0, 1, SUB], dtype=np.uint16)
    out = C.c_int32(-1)
    rc = _lib.lib().srhip_loss_expr_create_ex(kind.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              arg.ctypes.data_as(C.POINTER(C.c_uint16)), 3, None, 0, flags, C.byref(out))
    return rc, out.value


def test_flag_validation():
    rc0, h0 = create_ex(0)
    rc1, h1 = create_ex(K.LOSS_EXPR_TREE_CODE)
    assert rc0 == 0 and rc1 == 0 and h1 == h0 + 1 and K.LOSS_EXPR_TREE_CODE == 1
    for flags in (2, 3):  # refused before anything is registered: the next handle follows h1
        assert create_ex(flags) == (_lib.ERR_INVALID, -1), flags
    rc2, h2 = create_ex(0)
    assert rc2 == 0 and h2 == h1 + 1
    for h in (h0, h1, h2):
        assert _lib.lib().srhip_loss_expr_destroy(h) == 0


@pytest.mark.parametrize("name", ["E1", "E3", "E5"])
def test_the_flag_leaves_the_host_values_alone(name):
    lo = E.loss_options()
    plain, flagged = srhip.ExprLoss(E.EXPRS[name](lo), lo), srhip.ExprLoss(E.EXPRS[name](lo), lo, tree_code=True)
    assert flagged.tree_code and not plain.tree_code and flagged.kind != plain.kind
    assert srhip.Options(binary_operators=["+"], elementwise_loss=flagged).elementwise_loss is flagged
    rng = np.random.default_rng(5)
    yhat, y = rng.standard_normal((2, 500)).astype(np.float32)
    w = np.abs(rng.standard_normal(500)).astype(np.float32)
    with np.errstate(all="ignore"):
        np.testing.assert_array_equal(flagged.value(yhat, y, w), plain.value(yhat, y, w))


def test_prototype_and_julia_ccall_match_the_header():
    protos = header_prototypes()
    ret, args = protos["srhip_loss_expr_create_ex"]
    assert hasattr(_lib.lib(), "srhip_loss_expr_create_ex")
    assert len(_lib.SIGNATURES["srhip_loss_expr_create_ex"]) == len(args) == len(protos["srhip_loss_expr_create"][1]) + 1
    calls = {c[0]: c for c in julia_ccalls()}
    _, jret, jargs, _ = calls["srhip_loss_expr_create_ex"]
    assert _jl_kind(jret) == _c_kind(ret)
    assert [_jl_kind(a) for a in jargs] == [_c_kind(a) for a in args]
    src = JL.read_text()
    assert re.search(r"^function ExprLoss\(tree::Node\{T\}, operators; tree_code::Bool=false\)", src, re.M)
    assert re.search(r"^const SRHIP_LOSS_EXPR_TREE_CODE = UInt32\(1\)", src, re.M)
