"""Expression losses as loss tree code (srhip.ExprLoss(..., tree_code=True), jit.cpp
Gen::emit_loss_expr): the expression compiled by the tree compiler and run at the end of every tile
of every tree of a Float32 program. Every case builds 320 trees, above the 256 at which a program
gets tree code, and asserts that the tree code ran (last_tree_code() > 0).

References: the oracle applied twice (tests/expr_loss_cases.py) summed in float64, and the same
program's interpreted result through an unflagged handle of the same expression.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine opens the device: the process then holds one HIP runtime)

import expr_loss_cases as E
import oracle
import srhip
from srhip import _lib
from srhip.engine import _p

pytestmark = pytest.mark.gpu
T = np.float32
NTREES = 320


@functools.lru_cache(maxsize=None)
def handles(name):
    """(flagged, unflagged) handles of one expression, one pair per process."""
    lo = E.loss_options()
    return srhip.ExprLoss(E.EXPRS[name](lo), lo, tree_code=True), E.expr_loss(name)


def run(ctx, prog, ds, loss, tree_code):
    s, wsum, ok = prog.eval_loss(ds, loss.kind, loss.params)
    ran = ctx.last_tree_code()
    assert (ran > 0) if tree_code else (ran == 0), (loss, ran, ctx.last_kernel_name())
    return s, wsum, np.asarray(ok).astype(bool)


@functools.lru_cache(maxsize=None)
def exact_problem(n):
    """+ - * trees with constants in -2..2 over features in {-1, 0, 1}, y in -3..3, w in {1, 2, 3}.
    With the oracle on the CPU: all 320 trees succeed, |ŷ| <= 24, and Σ|ℓ| is at most 7 949 464
    (WSQ, n = 40 001) < 2^24, so every ℓ and every partial sum in any order is an exact Float32."""
    o = srhip.Options(binary_operators=["+", "-", "*"], unary_operators=[])
    flat = srhip.flatten(srhip.random_population(NTREES, o, 5, T, seed=31), o, dtype=T)
    flat.consts[:] = np.clip(np.rint(flat.consts), -2, 2)
    rng = np.random.default_rng(32)
    X = rng.integers(-1, 2, (5, n)).astype(T)
    y = rng.integers(-3, 4, n).astype(T)
    w = rng.integers(1, 4, n).astype(T)
    yhat, ok = oracle.eval_trees(flat, X, dtype=T)
    return flat, X, y, w, yhat, ok


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("n", [300, 40_001])
def test_exact_sums(gpu_ctx, n, weighted):
    """SQ, ABS and WSQ (on the weighted dataset) bit for bit against the float64 reference: n = 300
    is one full 256-row tile and one partial tile, n = 40 001 plans more than one row group."""
    flat, X, y, w, yhat, rok = exact_problem(n)
    ds = srhip.DeviceDataset(gpu_ctx, X, y, w if weighted else None)
    prog = srhip.Program(gpu_ctx, flat, T)
    for name in ("SQ", "ABS", "WSQ") if weighted else ("SQ", "ABS"):
        s, wsum, ok = run(gpu_ctx, prog, ds, handles(name)[0], True)
        if n > 300:
            assert gpu_ctx.last_loss_launch()["nrg"] > 1
        ref, mag = E.reference_sums(name, yhat, y, w, rok, T)
        assert np.nanmax(mag) < 2 ** 24
        assert np.array_equal(ok, rok) and rok.all()
        np.testing.assert_array_equal(s, ref, err_msg=name)
        assert wsum == (float(w.astype(np.float64).sum()) if weighted else float(n))


@pytest.mark.parametrize("n", [300, 40_001])
def test_parity_on_problem_a(gpu_ctx, n):
    """E1-E4 on problem A (+ - * / trees: no FAST rounding), weighted: ok is the oracle's on every
    tree, and |Σℓ - ref| <= 1e-5·Σ|ℓ| against the oracle's sums and against the interpreted result
    of an unflagged handle. 317 of the 320 trees succeed; E1 is non-finite on one more at 40 001."""
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, n, ntrees=NTREES)
    ds = srhip.DeviceDataset(gpu_ctx, X, y, w)
    prog = srhip.Program(gpu_ctx, flat, T)
    for name in ("E1", "E2", "E3", "E4"):
        flagged, plain = handles(name)
        s, _, ok = run(gpu_ctx, prog, ds, flagged, True)
        si, _, oki = run(gpu_ctx, prog, ds, plain, False)
        ref, mag = E.reference_sums(name, yhat, y, w, rok, T)
        assert np.array_equal(ok, rok) and np.array_equal(oki, rok), name
        m = rok & np.isfinite(ref)
        assert NTREES - int(m.sum()) < NTREES // 10, name
        err, erri = np.abs(s[m] - ref[m]), np.abs(s[m] - si[m])
        print(f"{name} n={n}: worst err/Σ|ℓ| oracle {float(np.max(err / mag[m])):.3g}, interpreter {float(np.max(erri / mag[m])):.3g}")
        assert np.all(err <= 1e-5 * mag[m]), (name, np.flatnonzero(m)[~(err <= 1e-5 * mag[m])][:10])
        assert np.all(erri <= 1e-5 * mag[m]), (name, np.flatnonzero(m)[~(erri <= 1e-5 * mag[m])][:10])


def test_fast_population(gpu_ctx):
    """The operator set of tests/test_jit_losses_gpu.py (cos, exp: FAST tiles) at n = 40 001 with E3
    (reads w) and E4 (ŷ twice): ok equals the oracle's and the interpreter's, sums within 1e-5
    relative of the interpreted result of the same expression on every tree that succeeds with a
    finite interpreted sum. With the oracle on the CPU: 260 of the 320 trees succeed, and E3 is finite
    on 257 of them."""
    n = 40_001
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    rng = np.random.default_rng(71)
    X = rng.standard_normal((5, n)).astype(T)
    y = (T(2) * np.cos(X[3]) + X[0] * X[0] - T(2)).astype(T)
    w = np.abs(rng.standard_normal(n)).astype(T)
    flat = srhip.flatten(srhip.random_population(NTREES, o, 5, T, seed=72), o, dtype=T)
    _, _, rok = oracle.eval_loss_batch(flat, X, y, dtype=T, nthreads=16)
    ds = srhip.DeviceDataset(gpu_ctx, X, y, w)
    prog = srhip.Program(gpu_ctx, flat, T)
    assert prog.jit_info()["nfast"] > 0
    for name in ("E3", "E4"):
        flagged, plain = handles(name)
        s, _, ok = run(gpu_ctx, prog, ds, flagged, True)
        si, _, oki = run(gpu_ctx, prog, ds, plain, False)
        assert np.array_equal(ok, rok) and np.array_equal(oki, rok), name
        m = rok & np.isfinite(si)
        assert NTREES - int(m.sum()) < 2 * NTREES // 3, (name, int(m.sum()))
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.abs(s - si) / np.abs(si)
        print(f"{name}: {int(m.sum())} trees, worst relative difference {float(np.max(rel[m])):.3g}")
        assert np.all(rel[m] <= 1e-5), (name, np.flatnonzero(m & ~(rel <= 1e-5))[:10])


def test_a_non_finite_loss_does_not_fail_the_tree(gpu_ctx):
    """E5 is NaN wherever p and t differ in sign: every succeeding tree of problem A gets a
    non-finite sum with ok = 1, and the three trees that fail in the interpreter fail here. None of
    E5's routines marks a finite input, so tanh(E5) runs too: tanh is handed the NaN and marks it
    (an operator that can turn a non-finite input finite does), and that mark must not reach the
    tree's verdict."""
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, 300, ntrees=NTREES)
    ds = srhip.DeviceDataset(gpu_ctx, X, y)
    prog = srhip.Program(gpu_ctx, flat, T)
    lo = E.loss_options()
    marked = lo.make_unary("tanh", E.e5(lo))
    for flagged, plain in (handles("E5"), (srhip.ExprLoss(marked, lo, tree_code=True), srhip.ExprLoss(marked, lo))):
        s, _, ok = run(gpu_ctx, prog, ds, flagged, True)
        _, _, oki = run(gpu_ctx, prog, ds, plain, False)
        assert np.array_equal(ok, rok) and np.array_equal(oki, rok) and int(rok.sum()) == 317
        assert not np.isfinite(s[rok]).any() and np.isnan(s[~rok]).all()


def test_weight_contract(gpu_ctx):
    """No implicit weight: SQ on the weighted dataset equals SQ on the unweighted one bit for bit
    while out_weight_sum is Σ w; WSQ differs."""
    flat, X, y, w, yhat, rok = exact_problem(300)
    prog = srhip.Program(gpu_ctx, flat, T)
    plain, weighted = srhip.DeviceDataset(gpu_ctx, X, y), srhip.DeviceDataset(gpu_ctx, X, y, w)
    su, wu, _ = run(gpu_ctx, prog, plain, handles("SQ")[0], True)
    sw, ww, _ = run(gpu_ctx, prog, weighted, handles("SQ")[0], True)
    sx, _, _ = run(gpu_ctx, prog, weighted, handles("WSQ")[0], True)
    np.testing.assert_array_equal(sw, su)
    assert wu == 300.0 and ww == float(w.astype(np.float64).sum())
    assert np.sum(sx != su) > NTREES // 2


def test_varying_constants(gpu_ctx):
    """A SRHIP_PROGRAM_VARYING_CONSTANTS program (constants read from memory): after set_constants
    the sums of E1 equal a fresh literal program's built on the new constants, so the candidates'
    constants moved and the loss's own 2.5 did not."""
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, 300, ntrees=NTREES)
    ds = srhip.DeviceDataset(gpu_ctx, X, y, w)
    new = (flat.consts * T(1.25) + T(0.5)).astype(T)
    vary = srhip.Program(gpu_ctx, flat, T, varying_constants=True)
    flagged = handles("E1")[0]
    s0, _, _ = run(gpu_ctx, vary, ds, flagged, True)
    vary.set_constants(new)
    s1, _, ok1 = run(gpu_ctx, vary, ds, flagged, True)
    flat2 = srhip.flatten(trees, o, dtype=T)
    flat2.consts[:] = new
    s2, _, ok2 = run(gpu_ctx, srhip.Program(gpu_ctx, flat2, T), ds, flagged, True)
    assert np.array_equal(ok1, ok2)
    np.testing.assert_array_equal(s1[ok1], s2[ok2])
    assert np.sum(s1[ok1] != s0[ok1]) > NTREES // 2


def test_what_stays_interpreted(gpu_ctx):
    """On one program: an unflagged handle runs no tree code; a flagged loss the tree compiler
    has no form for ((2 + 3)·(p - t): an operator on constants alone) runs interpreted with the
    results of its unflagged twin; a destroyed flagged handle is an invalid argument."""
    flat, X, y, w, yhat, rok = exact_problem(300)
    ds = srhip.DeviceDataset(gpu_ctx, X, y)
    prog = srhip.Program(gpu_ctx, flat, T)
    run(gpu_ctx, prog, ds, handles("SQ")[0], True)
    run(gpu_ctx, prog, ds, handles("SQ")[1], False)
    lo = E.loss_options()
    tree = lo.make_binary("*", lo.make_binary("+", srhip.Node(val=2.0), srhip.Node(val=3.0)),
                          lo.make_binary("-", srhip.Node("x1"), srhip.Node("x2")))
    a, b = srhip.ExprLoss(tree, lo, tree_code=True), srhip.ExprLoss(tree, lo)
    sa, _, oka = run(gpu_ctx, prog, ds, a, False)
    sb, _, okb = run(gpu_ctx, prog, ds, b, False)
    np.testing.assert_array_equal(sa, sb)
    np.testing.assert_array_equal(sa, 5.0 * (yhat.astype(np.float64) - y).sum(axis=1))
    a.destroy()
    sums, oks, ws = np.full(NTREES, -7.0), np.full(NTREES, 9, dtype=np.uint8), C.c_double(-7.0)
    rc = _lib.lib().srhip_eval_loss(ds.handle, prog.handle, a.kind, None, None, 0, _p(sums), C.byref(ws), _p(oks))
    assert rc == _lib.ERR_INVALID
    assert np.all(sums == -7.0) and np.all(oks == 9) and ws.value == -7.0  # the outputs are untouched
