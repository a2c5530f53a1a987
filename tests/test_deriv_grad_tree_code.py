"""The objective's gradient tree code on the CPU (csrc/jit_grad.cpp GradGen::dg, DESIGN.md
§3.19.1): the generator's bytes against llvm-mc's assembly of its own text."""
import pytest

import srhip
from srhip.engine import jit_compile
from test_deriv_tree_code import flat
from test_jit import LLVM, assemble, trans_forwarding_hazards


@pytest.mark.skipif(not (LLVM / "llvm-mc").exists(), reason="llvm-mc not installed")
@pytest.mark.parametrize("huber", [False, True], ids=["L2", "Huber"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dirs", ([0], [1, 0]), ids=str)
@pytest.mark.parametrize("k", [0, 1])
def test_machine_code_equals_llvm_mc(k, dirs, weighted, huber):
    loss = srhip.HuberLoss(0.7) if huber else None
    code, text, offs = jit_compile(flat(k), deriv=(dirs, 5, weighted), loss=loss, deriv_grad=True)
    print(f"{len(offs)} of 40 trees compiled")
    assert len(offs) >= 20  # (the pool holds values for two reverse sweeps: deep trees are refused)
    assert assemble(text) == code
    assert not trans_forwarding_hazards(text)
    # per tree: the channel partials and (a tree with constants) theirs, one vector store each
    assert len(offs) <= text.count("global_store_dword") <= 2 * len(offs)
