"""SRHIP_PROGRAM_EXPR_OP_TREE_CODE without a device: the flag's value in the header and both
bindings, the compile hook that takes it, and srhip_program_create_ex's flag mask."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

import expr_op_cases as E
import srhip
from srhip import _lib
from srhip import constants as K
from srhip.engine import jit_compile

ROOT = Path(__file__).resolve().parents[1]


def test_flag_value_in_header_and_bindings():
    hdr = (ROOT / "include" / "srhip.h").read_text()
    jl = (ROOT / "symbolicregression.jl_amd" / "julia" / "SRHip.jl").read_text()
    flag = int(re.search(r"#define SRHIP_PROGRAM_EXPR_OP_TREE_CODE (0x[0-9a-f]+)u", hdr).group(1), 16)
    assert flag == K.PROGRAM_EXPR_OP_TREE_CODE == 0x80  # (8 and 0x10 stay unknown bits: tests/test_wide_tree_code_gpu.py)
    assert int(re.search(r"const PROGRAM_EXPR_OP_TREE_CODE = UInt32\((\d+)\)", jl).group(1)) == flag
    assert "expr_op_tree_code ? PROGRAM_EXPR_OP_TREE_CODE" in jl


def test_hook_compiles_operator_trees_only_with_the_flag():
    """With the flag the hook returns offsets for the trees that hold operators (literal and
    memory-constant code, the threaded code generation's bytes equal to the text path's); without
    it the answer is srhip_jit_compile's, which leaves them out."""
    o, trees, flat, xflat, X, y, w = E.problem(np.float32, 256)
    is_op = (flat.kind >= K.NODE_UNARY) & (flat.arg >= K.EXPR_OP_BEGIN)
    hold = {t for t in range(flat.ntrees) if is_op[flat.node_off[t]:flat.node_off[t + 1]].any()}
    plain = jit_compile(flat, fast=True)
    assert len(hold) == 216 and len(plain[2]) == 59  # (the operators of 25 trees fold away)
    tr = srhip.engine._trees_struct(flat, np.ascontiguousarray(flat.consts, dtype=np.float32))
    n = [C.c_int64(len(plain[0])), C.c_int64(len(plain[1]) + 1), C.c_int64(2 * len(plain[2]))]
    buf, txt, off = np.zeros(n[0].value, np.uint8), C.create_string_buffer(n[1].value), np.zeros(n[2].value, np.int32)
    assert _lib.lib().srhip_jit_compile_ex(C.byref(tr), 1, 0, buf.ctypes.data, C.byref(n[0]), txt, C.byref(n[1]),
                                           off.ctypes.data, C.byref(n[2])) == 0
    assert bytes(buf) == plain[0] and txt.value.decode() == plain[1]
    for memc in (False, True):
        code, text, offs = jit_compile(flat, fast=True, memc=memc, expr_ops=True)
        assert hold <= set(offs) and len(offs) == 250
        assert "v_pk_fma_f32" in text and len(text.splitlines()) > len(plain[1].splitlines())
        assert jit_compile(flat, fast=True, memc=memc, expr_ops=True, text=False)[0] == code


def test_create_ex_still_refuses_unknown_flag_bits():
    tr = srhip.engine.Trees()
    out = C.c_void_p()
    assert _lib.lib().srhip_program_create_ex(C.c_void_p(1), 0, C.byref(tr), 0x10, C.byref(out)) == _lib.ERR_INVALID
    assert "unknown program flags" in _lib.lib().srhip_last_error().decode()


def test_program_sets_the_bit(monkeypatch):
    seen = []
    monkeypatch.setattr(srhip.engine, "check", lambda rc: None)

    class Lib:
        def srhip_program_create_ex(self, ctx, dtype, tr, flags, out):
            seen.append(flags)
            return 0

    monkeypatch.setattr(srhip.engine, "lib", lambda: Lib())
    flat = E.problem(np.float32, 256)[2]
    ctx = type("Ctx", (), {"handle": None})()
    for kw, want in (({}, 0), ({"expr_op_tree_code": True}, 0x80), ({"expr_op_tree_code": True, "varying_constants": True}, 0x81)):
        p = srhip.Program(ctx, flat, np.float32, **kw)
        p.handle = None
        assert seen[-1] == p.flags == want
