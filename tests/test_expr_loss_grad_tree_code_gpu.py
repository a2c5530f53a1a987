"""Expression losses in the reverse-mode gradient tree code (srhip.ExprLoss(..., grad_tree_code=True),
DESIGN.md §3.12.2) against NumPy float64 on an all-integer problem, bit for bit, and against the oracle's
∂ŷ/∂c times the analytic seed under the bound of tests/test_expr_loss_gpu.py. Every program holds at
least 256 trees (a gradient program then gets tree code) and every case asserts that tree code ran."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine opens the device: the process then holds one HIP runtime)

import expr_loss_cases as E
import oracle
import srhip
from srhip import _lib
from srhip.distributed import RowShardedEvaluator
from srhip.engine import _p
from test_expr_loss_gpu import SEEDS, const_grads, reference
from test_expr_loss_grad_tree_code import EXPRS, LOSS_OPS
from test_expr_loss_tree_code_gpu import exact_problem
from test_margin_losses_gpu import RTOL, check_sums

pytestmark = pytest.mark.gpu
T = np.float32
NTREES = 320


@functools.lru_cache(maxsize=None)
def handles(name):
    """(flagged, unflagged) handles of one expression, one pair per process."""
    o = srhip.Options(**LOSS_OPS)
    return srhip.ExprLoss(EXPRS[name](o), o, grad_tree_code=True), srhip.ExprLoss(EXPRS[name](o), o)


def run(ctx, prog, ds, loss, tree_code=True):
    s, g, wsum, ok = prog.eval_loss_grad(ds, loss.kind, loss.params)
    ran = ctx.last_tree_code()
    assert (ran > 0) if tree_code else (ran == 0), (loss, ran, ctx.last_kernel_name())
    return s, g, np.asarray(ok).astype(bool)


# ℓ and dℓ/dŷ of the exact cases in float64 (p, t, w integer-valued)
EXACT = {"SQ": (lambda p, t, w: (p - t) ** 2, lambda p, t, w: 2 * (p - t)),
         "WSQ": (lambda p, t, w: w * (p - t) ** 2, lambda p, t, w: 2 * w * (p - t)),
         "D2": (lambda p, t, w: (p - t) * (p + t), lambda p, t, w: 2 * p)}


@functools.lru_cache(maxsize=None)
def exact_grads(n):
    """∂ŷ/∂c of every tree of the exact problem by the oracle in float64 ([nconst, n] per tree; integers)."""
    flat, X, y, w, yhat, rok = exact_problem(n)
    out = []
    for t in range(flat.ntrees):
        k, ar, c = flat.tree(t)
        out.append(oracle.eval_grad_consts(k, ar, c.astype(np.float64), X.astype(np.float64), len(c), dtype=np.float64)[1]
                   if len(c) else np.zeros((0, n)))
    return out


@pytest.mark.parametrize("n", [300, 2049])
@pytest.mark.parametrize("name", ["SQ", "WSQ", "D2"])
def test_exact_sums_and_gradients(gpu_ctx, name, n):
    """Integers under + - *: every ℓ, seed, adjoint and partial sum is an integer below 2^24, so sums and
    gradients equal float64 bit for bit. n = 300: a full and a partial tile; 2049 crosses a row group."""
    flat, X, y, w, yhat, rok = exact_problem(n)
    ds = srhip.DeviceDataset(gpu_ctx, X, y, w if name == "WSQ" else None)
    s, g, ok = run(gpu_ctx, srhip.Program(gpu_ctx, flat, T), ds, handles(name)[0])
    assert np.array_equal(ok, rok) and rok.all()
    p, t64, w64 = yhat.astype(np.float64), y.astype(np.float64), w.astype(np.float64)
    lfn, sfn = EXACT[name]
    np.testing.assert_array_equal(s, lfn(p, t64, w64).sum(axis=1), err_msg=name)
    gref, mag = np.zeros_like(g), 0.0
    for tr, gc in enumerate(exact_grads(n)):
        term = sfn(p[tr], t64, w64) * gc
        gref[flat.const_off[tr]:flat.const_off[tr + 1]] = term.sum(axis=1)
        mag = max(mag, float(np.abs(term).sum(axis=1).max(initial=0.0)))
    assert mag < 2 ** 24 and len(g) > 600
    np.testing.assert_array_equal(g, gref, err_msg=name)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("name", ["E1", "E2"])
def test_parity_on_random_trees(gpu_ctx, name, weighted):
    """The problem and the bound of tests/test_expr_loss_gpu.py test_gradients_match_the_reference, unchanged:
    rtol·Σ|terms| plus the effect of a 4-ulp move of r on the seed; loss sums under check_sums."""
    n = 3001
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, n, 400, 82)
    rtol, eps = RTOL[np.dtype(T)], float(np.finfo(T).eps)
    ds = srhip.DeviceDataset(gpu_ctx, X, y, w if weighted else None)
    s, g, ok = run(gpu_ctx, srhip.Program(gpu_ctx, flat, T), ds, handles(name)[0])
    assert np.array_equal(ok, rok)
    ref, mag = reference(name, T, n, weighted, extra_deep=False, ntrees=400, seed=82)
    check_sums(s, ref, mag, float(n), ok & np.isfinite(ref), T, f"grad tree code {name}")
    y64, w64 = y.astype(np.float64), w.astype(np.float64)
    checked, worst = 0, 0.0
    for t, gc in const_grads(T, n).items():
        lo, hi = flat.const_off[t], flat.const_off[t + 1]
        with np.errstate(all="ignore"):
            r64 = (yhat[t] - y).astype(np.float64)  # r in T
            seed = SEEDS[name](r64, y64, w64)
            term = seed * gc
            d = (4 * eps * np.abs(r64)).astype(T).astype(np.float64)
            dv = np.maximum(np.abs(SEEDS[name](r64 + d, y64, w64) - seed),
                            np.abs(SEEDS[name](r64 - d, y64, w64) - seed)) * np.abs(gc)
        S, G, DV = np.abs(term).sum(axis=1), term.sum(axis=1), dv.sum(axis=1)
        sel = np.isfinite(S) & (S < 1e20)
        with np.errstate(invalid="ignore"):
            err = np.abs(g[lo:hi] - G)
        bound = rtol * S + DV + 1e-30
        worst = max(worst, float(np.max(err[sel] / bound[sel], initial=0.0)))
        assert np.all(err[sel] <= bound[sel]), (name, t, err[sel].tolist(), bound[sel].tolist())
        checked += int(sel.sum())
    print(f"{name} weighted={weighted}: {checked} entries, worst err / bound {worst:.3g}")
    assert checked >= 300, checked


@pytest.mark.parametrize("name", ["E5", "EXPLOG"])
def test_a_non_finite_loss_does_not_fail_the_tree(gpu_ctx, name):
    """Problem A, two tiles: ok is the candidate's alone, the sum non-finite where the oracle's loss rows are.
    exp(log(p / t)) hands log's NaN to exp, which marks its input: the mark must not reach the verdict."""
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, 300, ntrees=NTREES)
    s, g, ok = run(gpu_ctx, srhip.Program(gpu_ctx, flat, T), srhip.DeviceDataset(gpu_ctx, X, y), handles(name)[0])
    assert np.array_equal(ok, rok) and int(rok.sum()) == 317
    lo = srhip.Options(**LOSS_OPS)
    k, a, c = srhip.flatten([EXPRS[name](lo)], lo, dtype=np.float64).tree(0)
    with np.errstate(all="ignore"):
        fin = np.array([oracle.eval_tree(k, a, c, np.stack([yhat[t], y, np.zeros_like(y)]), dtype=T)[1] for t in range(NTREES)])
    assert int((rok & ~fin).sum()) >= 250
    assert not np.isfinite(s[rok & ~fin]).any() and np.isfinite(s[rok & fin]).all() and np.isnan(s[~rok]).all()


def test_what_stays_interpreted(gpu_ctx):
    """No tree code and the unflagged twin's results bit for bit: flagged E3 and E4 (log1p, tanh), a Float64
    program, row sets. A destroyed flagged handle is an invalid argument and leaves the outputs alone."""
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, 300, ntrees=NTREES)
    ds = srhip.DeviceDataset(gpu_ctx, X, y, w)
    prog = srhip.Program(gpu_ctx, flat, T)
    run(gpu_ctx, prog, ds, handles("E2")[0])
    _, _, flat64, X64, y64, w64, _, _ = E.problem(np.float64, 300, ntrees=NTREES)
    ds64, prog64 = srhip.DeviceDataset(gpu_ctx, X64, y64, w64), srhip.Program(gpu_ctx, flat64, np.float64)
    rows = np.random.default_rng(3).integers(0, 300, (NTREES, 40))
    twins = [[run(gpu_ctx, prog, ds, h, False) for h in handles(name)] for name in ("E3", "E4")]
    twins.append([run(gpu_ctx, prog64, ds64, h, False) for h in handles("E2")])
    twins.append([prog.eval_loss_grad_rowsets(ds, h.kind, rows, h.params) for h in handles("E2")])
    assert gpu_ctx.last_tree_code() == 0
    for ra, rb in twins:
        for va, vb in zip(ra, rb):
            np.testing.assert_array_equal(va, vb)
    lo = srhip.Options(**LOSS_OPS)
    dead = srhip.ExprLoss(EXPRS["SQ"](lo), lo, grad_tree_code=True)
    dead.destroy()
    sums, grads, oks, ws = np.full(NTREES, -7.0), np.full(int(flat.const_off[-1]), -7.0), np.full(NTREES, 9, dtype=np.uint8), C.c_double(-7.0)
    rc = _lib.lib().srhip_eval_loss_grad(ds.handle, prog.handle, dead.kind, None, _p(sums), _p(grads), C.byref(ws), _p(oks))
    assert rc == _lib.ERR_INVALID
    assert np.all(sums == -7.0) and np.all(grads == -7.0) and np.all(oks == 9) and ws.value == -7.0


def test_set_constants_keeps_the_module(gpu_ctx):
    """After set_constants a flagged E2 gradient call equals a fresh program's bit for bit, tree code both times."""
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, 300, ntrees=NTREES)
    ds = srhip.DeviceDataset(gpu_ctx, X, y, w)
    new = (flat.consts * T(1.25) + T(0.5)).astype(T)
    prog = srhip.Program(gpu_ctx, flat, T)
    s0, g0, _ = run(gpu_ctx, prog, ds, handles("E2")[0])
    prog.set_constants(new)
    s1, g1, ok1 = run(gpu_ctx, prog, ds, handles("E2")[0])
    flat2 = srhip.flatten(trees, o, dtype=T)
    flat2.consts[:] = new
    s2, g2, ok2 = run(gpu_ctx, srhip.Program(gpu_ctx, flat2, T), ds, handles("E2")[0])
    assert np.array_equal(ok1, ok2)
    np.testing.assert_array_equal(s1, s2)
    np.testing.assert_array_equal(g1, g2)
    assert np.sum(s1[ok1] != s0[ok1]) > NTREES // 2


def test_constant_optimisation(gpu_ctx, monkeypatch):
    """Flagged E2 on the 20 trees of the interpreted optimiser test, through an evaluator on srhip.Program
    (SRHIP_GJIT=1: the sets are below 256 trees): every gradient phase ran tree code, no loss rises, some fall."""
    monkeypatch.setenv("SRHIP_GJIT", "1")
    _, trees, flat, X, y, w, yhat, rok = E.problem(T, 3000)
    loss = handles("E2")[0]
    o = srhip.Options(binary_operators=list(E.ARITH), unary_operators=[], elementwise_loss=loss)
    picked = [t.copy() for t, k in zip(trees, rok) if k and srhip.has_constants(t)][:20]
    ds, dev, ran = srhip.Dataset(X, y), srhip.DeviceDataset(gpu_ctx, X, y), []

    class Recording(RowShardedEvaluator):
        def loss_grad(self, consts):
            out = super().loss_grad(consts)
            ran.append(gpu_ctx.last_tree_code())
            return out

    def factory(cands):
        return Recording(srhip.Program(gpu_ctx, srhip.flatten(cands, o, dtype=T), T), dev, loss, lambda b: b, T)

    start, ok = srhip.eval_loss_batch_ok(picked, ds, o)
    assert ok.all()
    res = srhip.optimize_constants_batch(ds, picked, o, rng=np.random.default_rng(15), evaluator_factory=factory)
    got = np.asarray(res.losses).astype(T)
    assert ran and min(ran) > 0, ran
    assert np.all(got <= start) and np.any(got < start), (got, start)
