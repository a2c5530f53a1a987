"""Expression operators in the Float32 loss tree code (SRHIP_PROGRAM_EXPR_OP_TREE_CODE, DESIGN.md
§3.13.1): trees that hold an operator compiled under the opaque-function rules of srhip.h.

References: the oracle on the expanded trees (oracle_b of tests/test_expr_ops_gpu.py) where
expansion preserves did_succeed, and the same program built without the flag — the 16-slot
OPSET_EXPR interpreter, pinned to the oracle by tests/test_expr_ops_gpu.py — everywhere. Bounds:
check_sums / RTOL of tests/test_margin_losses_gpu.py against the oracle; 1e-5 relative against the
interpreted program; bit equality where both sides run the same code.
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine opens the device: the process then holds one HIP runtime)

import expr_op_cases as E
import oracle
import srhip
from srhip import Node
from srhip import constants as K
from srhip.engine import jit_compile
from test_expr_ops_gpu import ORACLE_CONDITIONED, ORACLE_COUNTS, oracle_b
from test_margin_losses_gpu import check_sums, program

pytestmark = pytest.mark.gpu

T = np.float32
L2 = K.LOSS["L2"]
HUBER = srhip.HuberLoss(0.8)
REL = 1e-5


def flagged(ctx, flat, dtype=T, **kw):
    """The program with the flag, its loss tree code forced on as program(ctx, flat, T, "1") does."""
    os.environ["SRHIP_JIT"] = "1"
    try:
        return srhip.Program(ctx, flat, dtype, expr_op_tree_code=True, **kw)
    finally:
        del os.environ["SRHIP_JIT"]


def close_to_interpreted(s, ok, si, what):
    """Within 1e-5 relative of the interpreted sums on every succeeding tree with a finite sum."""
    m = ok & np.isfinite(si)
    rel = np.abs(s[m] - si[m]) / np.maximum(np.abs(si[m]), np.finfo(T).tiny)
    print(f"{what}: {int(m.sum())} trees, worst relative difference {rel.max() if rel.size else 0:.3g}")
    assert np.all(rel <= REL), (what, np.flatnonzero(m)[rel > REL][:10], rel[rel > REL][:10])
    assert np.array_equal(np.isfinite(s[ok]), np.isfinite(si[ok]))


TAILS = [pytest.param((L2, None, False), id="L2"), pytest.param((L2, None, True), id="L2-weighted"),
         pytest.param((HUBER.kind, HUBER.params, False), id="Huber")]


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("n", [1, 256, 513, 3000])
def test_operator_trees_in_tree_code_match_the_oracle(gpu_ctx, n, tail):
    """Problem B (non-lossy operators, 216 of 250 trees hold one): n = 1 a lone partial tile, 256 one
    exact tile, 513 a tile and a row, 3000 many tiles and a partial one. All 216 compile (counted on
    the CPU through srhip_jit_compile_ex). did_succeed is the oracle's on the expansions; L2 sums meet
    check_sums on the trees the oracle shows well conditioned; every tail is within 1e-5 relative of
    the interpreted program."""
    kind, par, weighted = tail
    o, trees, flat, xflat, X, y, w = E.problem(T, n)
    yhat, rok, rsum, lok, cond = oracle_b(T, n)
    assert (int(rok.sum()), int((~rok).sum())) == ORACLE_COUNTS[T][n] and np.array_equal(rok, lok)
    assert int(cond.sum()) == ORACLE_CONDITIONED[T][n]
    assert rok.sum() >= flat.ntrees // 2 and (~rok).sum() >= 5
    is_op = (flat.kind >= K.NODE_UNARY) & (flat.arg >= K.EXPR_OP_BEGIN)
    hold = [t for t in range(flat.ntrees) if is_op[flat.node_off[t]:flat.node_off[t + 1]].any()]
    compiled = jit_compile(flat, fast=True, expr_ops=True)[2]
    assert len(hold) == 216 and sum(t in compiled for t in hold) == 216
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, y, w if weighted else None)
    prog = flagged(ctx, flat)
    s, wsum, ok = prog.eval_loss(ds, kind, par)
    assert ctx.last_tree_code() == prog.pass_info()["tree_code"] == len(compiled) == flat.ntrees
    assert prog.jit_info()["nfast"] > 0
    assert np.array_equal(ok, rok)
    if kind == L2 and not weighted:
        nfin = check_sums(s, rsum, np.abs(rsum), float(n), rok & (cond | ~np.isfinite(rsum)), T, f"L2 n={n}")
        assert nfin == int(cond.sum())
    si, wi, oki = program(ctx, flat, T, "0").eval_loss(ds, kind, par)
    assert ctx.last_tree_code() == 0 and wi == wsum and np.array_equal(oki, ok)
    close_to_interpreted(s, ok, si, f"tail {kind} weighted={weighted} n={n}")
    assert np.isnan(s[~ok]).all()


def test_several_row_groups(gpu_ctx):
    """n = 40 001 plans more than one row group: verdicts are the oracle's on the expansions, sums
    within 1e-5 relative of the interpreted program."""
    n = 40001
    o, trees, flat, xflat, X, y, w = E.problem(T, n)
    with np.errstate(all="ignore"):
        _, _, rok = oracle.eval_loss_batch(xflat, X, y, dtype=T)
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, y)
    s, _, ok = flagged(ctx, flat).eval_loss(ds, L2)
    assert ctx.last_tree_code() == flat.ntrees and ctx.last_loss_launch()["nrg"] > 1
    assert np.array_equal(ok, rok) and rok.sum() >= flat.ntrees // 2 and (~rok).sum() >= 5
    si, _, oki = program(ctx, flat, T, "0").eval_loss(ds, L2)
    assert np.array_equal(oki, ok)
    close_to_interpreted(s, ok, si, f"L2 n={n}")


@pytest.mark.parametrize("n", [1, 513])
def test_opaque_semantics_in_tree_code(gpu_ctx, n):
    """The five trees of test_opaque_semantics and nexp(cube(x1)·cube(x1)), whose argument overflows
    inline at x1 = 1e7 (a row of n = 513): only the argument mark can fail it. One row has x1 = 100,
    where exp overflows: nexp(x1) + x2 and exp(nexp(x1)) succeed (chk is put back after the body,
    whose inv was handed Inf), nexp(exp(x1)) fails (the argument is checked)."""
    o = E.options(("nexp", "ulog"), unary=("cos", "exp", "cube"))
    U, B = o.make_unary, o.make_binary
    cube = U("cube", Node("x1"))
    trees = [B("+", U("nexp", Node("x1")), Node("x2")),
             U("nexp", U("exp", Node("x1"))),
             U("ulog", Node("x1")),
             U("ulog", B("*", Node("x2"), Node("x2"))),
             U("exp", U("nexp", Node("x1"))),
             U("nexp", B("*", cube, cube.copy()))]
    X = np.random.default_rng(31).standard_normal((2, n)).astype(T)
    X[1] = np.abs(X[1]) + T(0.5)
    X[0, 7 if n > 7 else 0] = T(100.0)
    if n > 1:
        X[0, 3], X[0, 5] = T(-2.0), T(1e7)
    neg, over = bool((X[0] < 0).any()), bool((np.abs(X[0]) > 1e6).any())
    flat = srhip.flatten(trees, o, dtype=T)
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, np.zeros(n, dtype=T))
    s, _, ok = flagged(ctx, flat).eval_loss(ds, L2)
    assert ctx.last_tree_code() == len(trees)
    assert ok.tolist() == [True, False, not neg, True, True, not over], (n, ok)
    si, _, oki = program(ctx, flat, T, "0").eval_loss(ds, L2)
    assert ctx.last_tree_code() == 0 and np.array_equal(oki, ok)
    close_to_interpreted(s, ok, si, f"opaque n={n}")


def test_lossy_operators_at_population_scale(gpu_ctx):
    """nexp, op2 (a body constant under a routine), dbl (its argument read three times) and ulog in
    250 random trees at n = 3000: did_succeed identical to the flag-off program's on every tree."""
    n = 3000
    o, trees, flat, xflat, X, y, w = E.problem(T, n, names=E.LOSSY + ("ulog",))
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = flagged(ctx, flat)
    s, _, ok = prog.eval_loss(ds, L2)
    assert ctx.last_tree_code() == prog.pass_info()["tree_code"] >= 198  # the operator trees srhip_jit_compile_ex takes
    si, _, oki = program(ctx, flat, T, "0").eval_loss(ds, L2)
    assert np.array_equal(oki, ok) and ok.sum() >= 50 and (~ok).sum() >= 5
    close_to_interpreted(s, ok, si, "lossy n=3000")


def test_memory_constant_code_follows_set_constants(gpu_ctx):
    """A varying_constants program over trees that each hold my_func_c (body constant 0.3) and op2
    (body constant 0.1; its inv keeps a tree on the PRECISE routines, where memory-constant and
    literal code compute the same bits): after set_constants(a·c + b) sums and verdicts equal a fresh
    literal-constant program's built on the new constants, bit for bit (body constants did not
    move), and most sums changed."""
    n = 513
    o, rnd, _, _, X, y, w = E.problem(T, n, names=("my_func_c", "op2"), xscale=1.0)
    trees = [o.make_binary("op2", t.copy(), o.make_binary("my_func_c", Node("x1"), Node(val=0.5 + 0.01 * k)))
             for k, t in enumerate(rnd)]
    flat = srhip.flatten(trees, o, dtype=T)
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = flagged(ctx, flat, varying_constants=True)
    before, _, okb = prog.eval_loss(ds, L2)
    nj = ctx.last_tree_code()
    assert nj >= 200
    new = (T(1.25) * flat.consts.astype(T) + T(0.5)).astype(T)
    prog.set_constants(new)
    after, _, oka = prog.eval_loss(ds, L2)
    assert ctx.last_tree_code() == nj and prog.update_stats()["inplace"] >= 1
    fs, _, fok = flagged(ctx, flat.take(np.arange(flat.ntrees), new)).eval_loss(ds, L2)
    assert ctx.last_tree_code() > 0
    assert np.array_equal(oka, fok) and np.array_equal(after, fs, equal_nan=True)
    both = oka & okb
    assert (after[both] != before[both]).sum() > flat.ntrees // 2


def test_what_stays_interpreted(gpu_ctx):
    """Flag off: a batch of operator trees runs no tree code. Flag on a Float64 program: the same
    results, no tree code. A tree whose values exhaust the register blocks — f(x, y) = (x·y)·(x + y)/4
    nested seven deep over computed leaves, every argument read twice — runs interpreted with the
    flag-off result bit for bit, beside compiled neighbours."""
    n = 513
    po = E.prim_options()
    x, y2 = Node("x1"), Node("x2")
    f = srhip.ExprOp("tc_f", po.make_binary("*", po.make_binary("*", po.make_binary("*", x, y2), po.make_binary("+", x.copy(), y2.copy())),
                                            Node(val=0.25)), po, 2)
    o = srhip.Options(binary_operators=["+", "-", "*", "/", f], unary_operators=["cos", "exp"])
    leaf = [0]

    def nest(d):
        if d == 0:
            leaf[0] += 1
            return o.make_unary("cos", o.make_binary("*", Node(val=0.1 * leaf[0]), Node(f"x{1 + leaf[0] % 2}")))
        return o.make_binary("tc_f", nest(d - 1), nest(d - 1))

    trees = [nest(1), nest(2), nest(7), o.make_binary("tc_f", Node("x1"), o.make_unary("exp", Node("x2")))]
    X = np.random.default_rng(81).standard_normal((2, n)).astype(T)
    yv = np.cos(X[0]).astype(T)
    ctx = gpu_ctx
    for dtype in (np.float32, np.float64):
        flat = srhip.flatten(trees, o, dtype=dtype)
        ds = srhip.DeviceDataset(ctx, X.astype(dtype), yv.astype(dtype))
        s0, _, ok0 = program(ctx, flat, dtype, "1").eval_loss(ds, L2)
        assert ctx.last_tree_code() == 0 and ok0.all()
        prog = flagged(ctx, flat, dtype)
        s1, _, ok1 = prog.eval_loss(ds, L2)
        if dtype == np.float64:
            assert ctx.last_tree_code() == 0 and np.array_equal(s1, s0) and np.array_equal(ok1, ok0)
            continue
        assert ctx.last_tree_code() == 3 and prog.pass_info()["deep"] == 1
        assert np.array_equal(ok1, ok0) and s1[2] == s0[2]
        close_to_interpreted(s1, ok1, s0, "register-pool neighbours")
    f.destroy()
