"""Derivative tree code on the CPU (csrc/jit_grad.cpp GradGen::dv): the
flag, the generator's bytes against llvm-mc's assembly of its own text, and the gradient
tree code of the same trees, which the mode must leave byte for byte."""
import hashlib

import numpy as np
import pytest

import srhip
from srhip import constants as K
from srhip.engine import jit_compile
from test_jit import GRAD_OPSETS, LLVM, assemble, trans_forwarding_hazards

DIRS = ([0], [2, 0], [0, 1, 2, 3])
# sha256 over (code bytes, sorted offsets) of jit_compile(flat(k), grad=True) built from the commit before
# the mode: the constant-gradient generator shares its rules with the mode and must not move.
# The third (the set with safe_log) is from the commit that made the LOG reverse rule scale its operand
# around v_rcp_f32, which flushes subnormals (found by tests/test_deriv_rows_gpu.py); a shared rule.
GRAD_SHA256 = (
    "6de0d6f4143aac5bbfa97a1323c4a1a807ab90582ec32f271357a3fc245d6c62",
    "99699e3f27ac022629a142be6d667a9300c46baf3c15081968dc53ae586ddcf4",
    "e9f3bbd96c73edcc9a93f58a55c6f974a94438d9b5e6e7e1986ac31eb4087523",
)


def flat(k):
    o = srhip.Options(binary_operators=GRAD_OPSETS[k][0], unary_operators=GRAD_OPSETS[k][1])
    return srhip.flatten(srhip.random_population(40, o, 5, np.float32, seed=31 + k), o, dtype=np.float32)


def test_flag_validates():
    assert K.PROGRAM_DERIV_TREE_CODE == 32
    fl = flat(0)
    # the hook's refusals: what srhip_eval_loss_deriv keeps in the interpreter
    with pytest.raises(srhip.SrhipError):
        jit_compile(fl, deriv=([0, 1, 2, 3, 4], 5, False))
    with pytest.raises(srhip.SrhipError):
        jit_compile(fl, deriv=([0], 5, False), loss=srhip.PeriodicLoss(2.0))
    with pytest.raises(srhip.SrhipError):
        jit_compile(fl, deriv=([5], 5, False))
    with pytest.raises(srhip.SrhipError):
        jit_compile(fl, deriv=([0], 62, True))  # 2 + 62 + 2 arrays: past the tile's literal offsets


@pytest.mark.skipif(not (LLVM / "llvm-mc").exists(), reason="llvm-mc not installed")
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dirs", DIRS, ids=str)
@pytest.mark.parametrize("k", range(len(GRAD_OPSETS)))
def test_machine_code_equals_llvm_mc(k, dirs, weighted):
    loss = None if k == 0 else srhip.HuberLoss(0.7)  # the inline L2 tail and a routine tail
    code, text, offs = jit_compile(flat(k), deriv=(dirs, 5, weighted), loss=loss)
    assert len(offs) >= 36, f"only {len(offs)} of 40 trees compiled"
    assert assemble(text) == code
    assert not trans_forwarding_hazards(text)
    # values leave through one vector store per tree
    assert text.count("global_store_dword") == len(offs)


@pytest.mark.parametrize("k", range(len(GRAD_OPSETS)))
def test_gradient_code_is_unchanged(k):
    code, _, offs = jit_compile(flat(k), grad=True)
    h = hashlib.sha256(code)
    h.update(repr(sorted(offs.items())).encode())
    assert h.hexdigest() == GRAD_SHA256[k]
