"""The trimmed root mark of the loss tree code (csrc/jit.cpp Gen,
SRHIP_JIT_TRIM_ROOT) on the CPU: with the knob on and off the machine code is
what llvm-mc makes of its text, and the knob changes what it says it changes
and nothing else.

Trees: config #2's seeded population (FAST trees with every kind of guard,
trees that read a shared column) and hand-made ones for the other paths: a
tree whose root is a leaf, a constant root (keeps the earlier root mark: the
constant block is the mark's temporary), a division-only FAST tree, and one
with a cancellation, an exp, a product and a cos of a FAST-derived value in
one tree. tests/test_jit_rotate_gpu.py checks on the GPU that the results do
not move by a bit."""
import os

import numpy as np
import pytest

import srhip
from srhip.engine import jit_compile
from test_jit import LLVM, assemble

KNOB = "SRHIP_JIT_TRIM_ROOT"
CFG2 = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
NAN_TEST = "v_cmp_u_f32_e32 vcc, v40, v40"     # chk against itself
ROOT_TEST = "v_cmp_u_f32_e32 vcc, v48, v49"    # the trimmed root mark's pair
GUARD_TEST = (("v_cmp_ngt_f32_e32 ", ", v45"), ("v_cmp_nle_f32_e32 ", ", v46"), ("v_cmp_nge_f32_e32 ", ", v47"),
              ("v_cmp_nge_f32_e32 ", ", v88"))  # the verdict's compares of the four accumulators


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def hand_made(o):
    N = srhip.Node
    x = lambda f: N(feature=f)
    B = o.make_binary
    # exp(c x_f): a constant inside, so that no shared column stands in for it
    e = lambda c, f: o.make_unary("exp", B("*", N(val=np.float32(c)), x(f)))
    # x2 / (cos(exp - exp x3) exp - x1): a cancellation, a product and a cos of FAST values on a divisor's path
    inner = B("-", e(1.1, 1), B("*", e(0.9, 2), x(3)))
    guards = B("/", x(2), B("-", B("*", o.make_unary("cos", inner), e(0.7, 5)), x(1)))
    return {"leaf": x(2), "constant": N(val=np.float32(1.5)), "division": o.make_binary("/", x(1), x(2)),
            "guards": guards}


def tree_text(text, offs, t):
    """The assembly of tree t (jit.cpp gen_tree marks each tree's start)."""
    parts = text.split("; tree code at ")
    mine = [p for p in parts[1:] if int(p.split("\n", 1)[0]) == offs[t]]
    assert len(mine) == 1
    return mine[0]


@pytest.fixture(scope="module")
def batch():
    o = srhip.Options(**CFG2)
    hm = hand_made(o)
    trees = list(hm.values()) + srhip.random_population(400, o, 5, np.float32, seed=1000)
    return srhip.flatten(trees, o, dtype=np.float32), {n: i for i, n in enumerate(hm)}


VARIANTS = [{}, {KNOB: "0"}]


@pytest.mark.skipif(not (LLVM / "llvm-mc").exists(), reason="llvm-mc not installed")
@pytest.mark.parametrize("kv", VARIANTS, ids=["on", "off"])
def test_machine_code_equals_llvm_mc(batch, kv):
    flat, ids = batch
    with env(**kv):
        for fast, memc in ((True, False), (False, False), (True, True)):
            code, text, offs = jit_compile(flat, fast=fast, memc=memc)
            assert all(t in offs for t in ids.values())
            assert assemble(text) == code, (kv, fast, memc)
            if not memc:  # some tree reads a shared column
                assert "global_load_dwordx4" in text


def test_the_knob_changes_the_root_mark_only(batch):
    flat, ids = batch
    texts = {}
    for kv in VARIANTS:
        with env(**kv):
            _, text, offs = jit_compile(flat, fast=True)
        texts[tuple(kv)] = {n: tree_text(text, offs, t) for n, t in ids.items()}
    on, off = texts[()], texts[(KNOB,)]
    tests = lambda s: [sum(ln.startswith(a) and ln.endswith(b) for ln in s.splitlines()) for a, b in GUARD_TEST]
    FAST = ("division", "guards")  # the leaf and the constant call no routine: PRECISE only, no verdict
    # every kind of guard is in the hand-made tree, tested once per tile either way
    assert tests(off["guards"]) == tests(on["guards"]) == [1, 1, 1, 1], off["guards"]
    # the earlier code: chk tested by a FAST tree's verdict and by every tail, the root folded into chk
    for n in ("leaf", "division", "guards"):
        assert off[n].count(NAN_TEST) == (2 if n in FAST else 1) and off[n].count(ROOT_TEST) == 0, (n, off[n])
        assert off[n].count("v_fma_f32 v40, ") == 2 and off[n].count("v_pk_fma_f32 v[48:49], ") == 1
    # trimmed: one test of the pair, chk written on the failing path only, no test in the tail
    mark = ("v_fma_f32 v40, ", "v_pk_fma_f32 v[48:49], ", "v_cmp_u_f32_e32 ", "v_mov_b32_e32 v40, 0x7fc00000")
    rest = lambda s: [ln for ln in s.splitlines() if ln.startswith(("v_", "ds_", "global_")) and not ln.startswith(mark)]
    for n in ("leaf", "division", "guards"):
        t = on[n]
        assert t.count(NAN_TEST) == 0 and t.count(ROOT_TEST) == 1, (n, t)
        assert t.count("v_fma_f32 v40, ") == 0 and t.count("v_pk_fma_f32 v[48:49], ") == 2
        assert t.count("v_mov_b32_e32 v40, 0x7fc00000") == 1
        # the failing path sets chk and returns: the last two instructions of the tree
        body = [ln for ln in t.splitlines() if ln != "s_nop 0"]
        assert body[-2:] == ["v_mov_b32_e32 v40, 0x7fc00000", "s_setpc_b64 s[76:77]"] or n in FAST, body[-4:]
        # every other vector and memory instruction is the earlier code's, in its order
        assert rest(t) == rest(off[n]), n
    # a constant root keeps the earlier mark
    strip = lambda s: [ln for ln in s.splitlines()[1:] if not ln.startswith(("s_add_u32 s86", "s_addc_u32 s87"))]
    assert strip(on["constant"]) == strip(off["constant"]) and on["constant"].count(NAN_TEST) == 1
