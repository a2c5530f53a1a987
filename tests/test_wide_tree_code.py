"""Wide loss tree code on the CPU (csrc/jit.cpp Options::xg): Float32
literal-constant loss code whose features come from X in device memory, one
global_load_dwordx4 per feature per tile through a bounded window of register blocks, and
whose LDS tile holds y and w only.

The batches are tests/wide_cases.py's problem(float32, nfeat, 700, 300): 300 random trees
plus 6 hand-made ones. 305 of the 306 are tree-code candidates (the deep hand-made tree needs
more than the shallow interpreter's slots), which is what the LDS code accepts once every
feature index is relabelled f mod 60; as they stand it accepts 122 at 160 features and 81 at
300 ("feature offset beyond the DS immediate"). The GPU tests
(tests/test_wide_tree_code_gpu.py) check what the code computes."""
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

import srhip
import wide_cases as W
from srhip import Node
from srhip import constants as K
from srhip.engine import jit_compile
from test_jit import LLVM, OPSETS, assemble

needs_mc = pytest.mark.skipif(not (LLVM / "llvm-mc").exists(), reason="llvm-mc not installed")
ROOT = Path(__file__).resolve().parent.parent

# sha256 over (code bytes, sorted offsets) of test_jit.py's three operator sets, each with
# (fast, memc) = (1, 0), (0, 0), (1, 1) and no wide bit: the values of the commit before the wide bit
# (DESIGN.md §3.14 records them beside that branch's), with two literals moved since: the LogCosh and
# LogitDist loss routines grew by 0x700 bytes per region (the loss forms), so the distance
# between the FAST and the PRECISE region that every call site holds went from 0x28f00 to 0x29600 and the
# pc-relative distance to the routines by twice that; same instructions, same lengths, same offsets
UNFLAGGED_SHA256 = (
    "798e746abde33dcd2baf6a6b8832577436d19b2658cfbcf30acf456b17287765",
    "d11e8a822cd5c25089ea9968b028abea580f4b28476c48e5795b137aebf58b29",
    "6ac33e347c82da6895b32b81506f80b2cb388f7bd5d6b2a93a2479a012dac42c",
)


def check_wide_text(text, what):
    """Features by global loads; of LDS only y (offset 0 at the lane's tile address) and w
    (at s_woff + that address): no ds_read_b128 carries a feature's immediate offset."""
    assert "global_load_dwordx4" in text, what
    reads = [ln for ln in text.splitlines() if "ds_read_b128" in ln]
    assert reads and not [ln for ln in reads if "offset" in ln], what
    assert {ln.split("],")[1].strip() for ln in reads} <= {"v41", "v48"}, what  # VLANE (y), VGT (w)


def check_bytes(code, text, what):
    ref = assemble(text)
    assert len(ref) == len(code), what
    if ref != code:
        a, r = np.frombuffer(code, dtype=np.uint32), np.frombuffer(ref, dtype=np.uint32)
        i = int(np.flatnonzero(a != r)[0])
        raise AssertionError(f"{what}: word {i}: jit {a[i]:#010x} vs llvm-mc {r[i]:#010x}")


@needs_mc
@pytest.mark.parametrize("nfeat,narrow", [(160, 122), (300, 81)])
def test_wide_code_compiles_the_batch_and_equals_llvm_mc(nfeat, narrow):
    o, trees, flat, X, y, w = W.problem(np.float32, nfeat, 700, 300)
    assert len(trees) == 306
    _, _, offs_lds = jit_compile(flat)
    assert len(offs_lds) == narrow  # what the LDS code accepts, as on the parent
    for fast in (True, False):
        code, text, offs = jit_compile(flat, fast=fast, wide=True)
        print(f"nfeat={nfeat} fast={fast}: {len(offs)} of {len(trees)} trees, {len(code)} bytes")
        assert 290 <= len(offs) <= 305
        assert all(v % 64 == 0 for v in offs.values())
        check_wide_text(text, f"nfeat={nfeat} fast={fast}")
        check_bytes(code, text, f"nfeat={nfeat} fast={fast}")


@needs_mc
def test_wide_code_with_a_loss_routine_equals_llvm_mc():
    o, trees, flat, X, y, w = W.problem(np.float32, 160, 700, 300)
    code, text, offs = jit_compile(flat, loss=srhip.HuberLoss(1.0), wide=True)
    assert 290 <= len(offs) <= 305
    check_wide_text(text, "Huber")
    check_bytes(code, text, "Huber")
    _, _, offs_lds = jit_compile(flat, loss=srhip.HuberLoss(1.0))
    assert len(offs_lds) == 122


def test_threaded_generation_of_wide_code_equals_serial():
    """1500 + 6 trees: past the 512 candidates from which build() generates on several threads."""
    o, trees, flat, X, y, w = W.problem(np.float32, 160, 700, 1500)
    code_t, _, offs_t = jit_compile(flat, wide=True)
    code_p, text_p, offs_p = jit_compile(flat, wide=True, text=False)
    assert text_p == "" and len(offs_t) >= 1450
    assert offs_p == offs_t and code_p == code_t


@needs_mc
def test_hand_made_trees_over_high_features():
    """x_64, x_65, x_66 are columns 63, 64 and 65: the last two inline constants of the
    column's stride multiplier and its first literal; x_256 and x_300 lie past the 256
    entries of the per-column tables, which wide code indexes by the tree's own feature
    numbers; and a tree of 12 distinct features, more than the 8 register blocks."""
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    B, U = o.make_binary, o.make_unary
    x = lambda f: Node(feature=f)  # noqa: E731
    twelve = x(70)
    for k in range(1, 12):
        twelve = B(("+", "*", "-")[k % 3], twelve, x(70 + 19 * k))
    trees = [x(64), B("*", x(65), x(66)), B("/", U("cos", x(66)), x(64)), B("+", U("exp", x(256)), Node(val=0.5)),
             B("-", B("*", x(300), x(300)), U("cos", x(1))), twelve]
    flat = srhip.flatten(trees, o, dtype=np.float32)
    # the LDS code refuses every tree that reads such a feature into a register block
    assert not {0, 1, 4, 5} & set(jit_compile(flat)[2])
    for fast in (True, False):
        code, text, offs = jit_compile(flat, fast=fast, wide=True)
        assert sorted(offs) == list(range(len(trees))), sorted(offs)
        check_wide_text(text, "hand-made")
        check_bytes(code, text, "hand-made")
        mults = set(re.findall(r"s_mul_i32 s2, s38, (\S+)", text))
        for col in (63, 64, 65, 255, 299):
            assert hex(col) in mults, (col, sorted(mults))
        # one load per distinct feature per tree and tile
        assert text.count("global_load_dwordx4") == 1 + 2 + 2 + 1 + 2 + 12


def test_wide_bit_has_no_effect_on_other_code():
    """Memory-constant and per-row output code are never wide: the bit changes nothing there."""
    o, trees, flat, X, y, w = W.problem(np.float32, 160, 700, 300)
    for kw in (dict(memc=True), dict(out=True)):
        assert jit_compile(flat, wide=True, **kw) == jit_compile(flat, **kw)


@pytest.mark.parametrize("k", range(len(OPSETS)))
def test_code_without_the_bit_is_the_parents(k):
    b_ops, u_ops = OPSETS[k]
    o = srhip.Options(binary_operators=b_ops, unary_operators=u_ops)
    flat = srhip.flatten(srhip.random_population(300, o, 7, np.float32, seed=11 + k), o, dtype=np.float32)
    h = hashlib.sha256()
    for fast, memc in ((True, False), (False, False), (True, True)):
        code, _, offs = jit_compile(flat, fast=fast, memc=memc)
        h.update(code)
        h.update(repr(sorted(offs.items())).encode())
    assert h.hexdigest() == UNFLAGGED_SHA256[k]


def test_flag_constants_and_keywords_match_the_header():
    """The flag's acceptance by srhip_program_create_ex needs a context, so a device: checked
    in tests/test_wide_tree_code_gpu.py. Here: one value in the header, Python and Julia, and
    the keyword on both Julia constructors and the Python ones."""
    hdr = (ROOT / "include" / "srhip.h").read_text()
    jl = (ROOT / "symbolicregression.jl_amd" / "julia" / "SRHip.jl").read_text()
    val = int(re.search(r"#define SRHIP_PROGRAM_WIDE_TREE_CODE (\d+)u", hdr).group(1))
    assert val == 4 == K.PROGRAM_WIDE_TREE_CODE
    assert int(re.search(r"const PROGRAM_WIDE_TREE_CODE = UInt32\((\d+)\)", jl).group(1)) == val
    others = [int(v) for v in re.findall(r"#define SRHIP_PROGRAM_\w+ (\d+)u", hdr)]
    assert sorted(others) == [1, 2, 4]  # distinct bits; 8 is unknown
    for ctor in ("function Program(", "function GroupProgram("):
        sig = jl[jl.index(ctor):]
        sig = sig[:sig.index("where {T}")]
        assert "wide_tree_code::Bool=false" in sig, ctor
        body = jl[jl.index(ctor):][:1500]
        assert "wide_tree_code ? PROGRAM_WIDE_TREE_CODE : UInt32(0)" in body, ctor
    import inspect

    from srhip.engine import GroupProgram, Program
    from srhip.interface import compile_trees

    for f in (Program.__init__, GroupProgram.__init__, compile_trees):
        assert inspect.signature(f).parameters["wide_tree_code"].default is False
