"""Margin (classification) losses on the GPU: the eleven LossFunctions.jl margin
losses L(a) on the agreement a = y·ŷ, y ∈ {-1, +1}, through every evaluation
path that takes a loss — the interpreters of both dtypes, the Float32 loss tree
code (a loss routine per margin id, the agreement in the tile tail), per-tree
minibatches, gradients (interpreted: margin losses have no gradient tree code)
and the constant optimiser — and the parameter rules of the C ABI.

The checker is tests/margin_reference.py (NumPy, written from the table of
include/srhip.h) applied to the oracle's per-row predictions: ŷ of `+ - * /`
trees is bit-exact by the project's own bar, so every kink and the ZeroOne
step fall on the same side in the engine and in the checker, and the bound
needs no spread allowance:

    |got - ref| <= rtol·Σ w|ℓ| + 4·eps(T)·Σ w,   rtol = 1e-5 (Float32), 1e-9 (Float64)

ref = Σ w·L(a) in float64 over the T-valued elementwise losses; the absolute
term is the rounding grain of loss values near 1 (1 - tanh a).
"""
import functools
import os

import numpy as np
import pytest

import margin_reference as M
import oracle
import srhip
from numerics import output_spread_flat
from srhip import _lib
from srhip import constants as K

pytestmark = pytest.mark.gpu

LOSSES = [srhip.ZeroOneLoss(), srhip.PerceptronLoss(), srhip.LogitMarginLoss(), srhip.L1HingeLoss(),
          srhip.L2HingeLoss(), srhip.SmoothedL1HingeLoss(0.5), srhip.ModifiedHuberLoss(), srhip.L2MarginLoss(),
          srhip.ExpLoss(), srhip.SigmoidLoss(), srhip.DWDMarginLoss(1.0)]
NAME = {K.LOSS[n]: n for n in M.NAMES}
# margin losses whose Float32 tree-code routine the generator left out (gen_jit.py's
# register-fit check): they run interpreted. None are.
NO_ROUTINE = set()
FINITE_F32_EXP = 90  # finite Float32 LogitMargin / Exp references at n = 3000: 92 by the checker alone
RTOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-9}
ARITH = (("+", "-", "*", "/"), ())
TRANSC = (("+", "-", "*", "/"), ("cos", "exp"))


@functools.lru_cache(maxsize=None)
def problem(T, n, ops=ARITH, ntrees=200, tree_seed=11):
    """Trees, data with y ∈ {-1, +1}, weights, and the oracle's per-row predictions
    (computed once per shape, shared and never written to)."""
    T = np.dtype(T).type
    o = srhip.Options(binary_operators=list(ops[0]), unary_operators=list(ops[1]))
    trees = srhip.random_population(ntrees, o, 5, T, seed=tree_seed)
    flat = srhip.flatten(trees, o, dtype=T)
    X = np.random.default_rng(12).standard_normal((5, n)).astype(T)
    y = np.where(2 * np.cos(X[3]) + X[0] * X[0] - 2 >= 0, 1, -1).astype(T)
    w = np.abs(np.random.default_rng(13).standard_normal(n)).astype(T)
    with np.errstate(all="ignore"):
        yhat, ok = oracle.eval_trees(flat, X, dtype=T)
    for a in (X, y, w, yhat, ok):
        a.setflags(write=False)
    return o, trees, flat, X, y, w, yhat, ok


def reference_sums(loss, yhat, y, w):
    """(Σ w·L(a), Σ w·|L(a)|) per tree in float64 over the T-valued elementwise losses, a = ŷ·y in T."""
    with np.errstate(all="ignore"):
        l = M.value(loss.kind, loss.param, yhat * y).astype(np.float64)
        if w is not None:
            l = l * w.astype(np.float64)
        return l.sum(axis=1), np.abs(l).sum(axis=1)


def check_sums(got, ref, mag, wsum, ok, T, what):
    """The module's bound on every succeeding tree; a non-finite reference (an exp overflow to
    +Inf, DWDMargin's 1/a at a = 0) is matched exactly. Returns the number of finite checks."""
    eps = float(np.finfo(T).eps)
    fin = ok & np.isfinite(ref)
    nf = ok & ~np.isfinite(ref)
    assert np.array_equal(got[nf], ref[nf], equal_nan=True), (what, got[nf][:5], ref[nf][:5])
    err = np.abs(got[fin] - ref[fin])
    bound = RTOL[np.dtype(T)] * mag[fin] + 4 * eps * wsum
    bad = np.flatnonzero(~(err <= bound))
    worst = float(np.max(err / bound)) if err.size else 0.0
    print(f"{what}: {int(fin.sum())} finite trees, {int(nf.sum())} non-finite, worst err/bound {worst:.3g}")
    assert bad.size == 0, (what, np.flatnonzero(fin)[bad][:10], err[bad][:10], bound[bad][:10])
    return int(fin.sum())


def program(ctx, flat, T, jit=None):
    """A program with the loss tree code forced on ("1") or off ("0"), or the default."""
    if jit is None:
        return srhip.Program(ctx, flat, T)
    os.environ["SRHIP_JIT"] = jit
    try:
        return srhip.Program(ctx, flat, T)
    finally:
        del os.environ["SRHIP_JIT"]


@pytest.mark.parametrize("n", [1, 256, 513, 3000])
@pytest.mark.parametrize("T,jit", [(np.float32, "0"), (np.float32, "1"), (np.float64, None)],
                         ids=["f32-interp", "f32-treecode", "f64"])
def test_all_margin_losses_match_the_reference(gpu_ctx, T, jit, n):
    """Strict parity of all eleven losses: n = 1 (a lone partial tile), 256 (one exact
    tree-code tile), 513 (an interpreter tile of 512 and one row), 3000 (many tiles, the
    last partial); weighted and not. Under SRHIP_JIT=1 the loss must have run as tree
    code (a silent fall-back fails). Unweighted ZeroOne sums equal the integer counts.

    Checked on the CPU with the oracle: 197 of 200 trees succeed at every n; at n = 3000
    at least 195 have a finite reference for every loss, but in Float32 only 92 for
    LogitMargin and Exp (105 trees have a row with a < -88.7, where Float32 exp(-a) is
    +Inf: those are checked to be +Inf, and at least 90 finite ones must remain; the other
    losses, and Float64, need 100); an emulation of the engine's arithmetic (NumPy
    elementwise in T, float64 sum) stays below 1e-2 of the bound."""
    o, trees, flat, X, y, w, yhat, rok = problem(T, n)
    ctx = gpu_ctx
    prog = program(ctx, flat, T, jit)
    for weights in (None, w):
        ds = srhip.DeviceDataset(ctx, X, y, weights)
        for loss in LOSSES:
            s, wsum, ok = prog.eval_loss(ds, loss.kind, loss.params)
            ran = ctx.last_tree_code()
            what = f"{NAME[loss.kind]} {np.dtype(T).name} jit={jit} n={n} weighted={weights is not None}"
            if jit == "1":
                assert (ran == 0) if NAME[loss.kind] in NO_ROUTINE else (ran > 0), (what, ran)
            else:
                assert jit is None or ran == 0, (what, ran)
            ok = np.asarray(ok).astype(bool)
            assert np.array_equal(ok, rok), what
            ref, mag = reference_sums(loss, yhat, y, weights)
            assert wsum == pytest.approx(float(n if weights is None else weights.astype(np.float64).sum()), rel=1e-6)
            nfin = check_sums(s, ref, mag, wsum, ok, T, what)
            if loss.kind == K.LOSS["ZEROONE"] and weights is None:
                assert np.array_equal(s[ok], ref[ok]), what  # integer counts, exactly
            if n == 3000:
                assert nfin >= (FINITE_F32_EXP if T == np.float32 and NAME[loss.kind] in ("LOGITMARGIN", "EXP")
                                else 100), (what, nfin)
        assert int(rok.sum()) == 197


@pytest.mark.parametrize("loss", [srhip.LogitMarginLoss(), srhip.L1HingeLoss(), srhip.ModifiedHuberLoss(),
                                  srhip.SigmoidLoss()], ids=lambda l: NAME[l.kind])
def test_tree_code_with_transcendental_trees(gpu_ctx, loss):
    """Tree code against the interpreter on trees with cos and exp (ŷ no longer bit-exact:
    the FAST path, 1-ulp transcendentals): within 1e-5·Σ w|ℓ| of each other, and both
    within the bound of the reference plus, per row, what a move of a by
    δ = 4·|y|·(the oracle's own output spread, tests/numerics.py) does to L — max - min of
    L over {a - δ, a, a + δ}. Trees whose summed allowance exceeds 1e-3·Σ w|ℓ| are
    ill-conditioned and left out: at most 20 % of the succeeding, finite trees (with the
    reference alone, unweighted: 10 % LogitMargin, 13 % L1Hinge, 14 % ModifiedHuber,
    7 % Sigmoid)."""
    T, n = np.float32, 3000
    o, trees, flat, X, y, w, yhat, rok = problem(T, n, TRANSC)
    ctx = gpu_ctx
    progs = {m: program(ctx, flat, T, m) for m in ("1", "0")}
    with np.errstate(all="ignore"):
        delta = 4 * np.abs(y.astype(np.float64)) * output_spread_flat(flat, X, T)
        a = (yhat * y).astype(np.float64)
        v = [M.value(loss.kind, loss.param, (a + d).astype(T)).astype(np.float64) for d in (-delta, 0 * delta, delta)]
        allow_row = np.maximum.reduce(v) - np.minimum.reduce(v)
    for weights in (None, w):
        ds = srhip.DeviceDataset(ctx, X, y, weights)
        s1, wsum, ok1 = progs["1"].eval_loss(ds, loss.kind, loss.params)
        assert ctx.last_tree_code() > 0
        s0, _, ok0 = progs["0"].eval_loss(ds, loss.kind, loss.params)
        assert ctx.last_tree_code() == 0
        ok1, ok0 = np.asarray(ok1).astype(bool), np.asarray(ok0).astype(bool)
        assert np.array_equal(ok1, rok) and np.array_equal(ok0, rok)
        ref, mag = reference_sums(loss, yhat, y, weights)
        w64 = np.ones(n) if weights is None else weights.astype(np.float64)
        with np.errstate(all="ignore"):
            allow = (allow_row * w64).sum(axis=1)
        fin = rok & np.isfinite(ref) & np.isfinite(s0)
        assert np.all(np.abs(s1[fin] - s0[fin]) <= 1e-5 * mag[fin]), NAME[loss.kind]
        keep = fin & (allow <= 1e-3 * mag)
        left_out = 1.0 - keep.sum() / fin.sum()
        print(f"{NAME[loss.kind]} weighted={weights is not None}: {int(fin.sum())} finite, left out {left_out:.1%}")
        assert left_out <= 0.20, (NAME[loss.kind], left_out)
        eps = float(np.finfo(T).eps)
        for got, name in ((s1, "tree code"), (s0, "interpreter")):
            err = np.abs(got[keep] - ref[keep])
            bound = 1e-5 * mag[keep] + 4 * eps * wsum + allow[keep]
            assert np.all(err <= bound), (name, NAME[loss.kind], np.flatnonzero(keep)[~(err <= bound)][:10])


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("loss", [srhip.L1HingeLoss(), srhip.LogitMarginLoss()], ids=lambda l: NAME[l.kind])
def test_per_tree_minibatches(gpu_ctx, T, loss):
    """srhip_eval_loss_rowsets: every tree on its own sample of 50 rows, drawn with
    replacement (repeats), one sample a single row repeated; the bound of this module per
    tree on its own sample."""
    n, bs = 3000, 50
    o, trees, flat, X, y, w, _, _ = problem(T, n)
    sub = srhip.flatten(trees[:50], o, dtype=T)
    rng = np.random.default_rng(14)
    rows = rng.integers(0, n, (sub.ntrees, bs))
    rows[0, :] = rows[0, 0]
    rows[1, : bs // 2] = rows[1, bs // 2:]
    assert any(len(set(r)) < bs for r in rows[2:])  # repeats within ordinary samples too
    # the oracle's predictions of each tree on its own sample
    with np.errstate(all="ignore"):
        per_tree = [oracle.eval_tree(*sub.tree(t), X[:, rows[t]], dtype=T) for t in range(sub.ntrees)]
    yh = np.stack([p[0] for p in per_tree])
    rok = np.array([p[1] for p in per_tree], dtype=bool)
    eps = float(np.finfo(T).eps)
    for weights in (None, w):
        ds = srhip.Dataset(X, y, weights=weights)
        dev = ds.device()
        prog = srhip.engine.Program(dev.ctx, sub, T)
        s, ws, ok = prog.eval_loss_rowsets(dev, loss.kind, rows, loss.params)
        assert np.array_equal(np.asarray(ok).astype(bool), rok)
        with np.errstate(all="ignore"):
            e = M.value(loss.kind, loss.param, yh * y[rows]).astype(np.float64)
        w64 = np.ones(rows.shape) if weights is None else weights[rows].astype(np.float64)
        wsum = w64.sum(axis=1)
        assert np.allclose(ws, wsum, rtol=1e-6)
        ref, mag = (e * w64).sum(axis=1), np.abs(e * w64).sum(axis=1)
        nf = rok & ~np.isfinite(ref)
        assert np.array_equal(s[nf], ref[nf], equal_nan=True)
        fin = rok & np.isfinite(ref)
        err = np.abs(s[fin] - ref[fin])
        bound = RTOL[np.dtype(T)] * mag[fin] + 4 * eps * wsum[fin]
        assert np.all(err <= bound), (NAME[loss.kind], np.flatnonzero(fin)[~(err <= bound)])
        assert fin.sum() >= 30


@functools.lru_cache(maxsize=None)
def const_grads(T, n):
    """The oracle's ∂ŷ/∂c in T (as float64) of every succeeding tree of the gradient problem
    that has constants: {tree: [nconst, n]}, computed once per dtype."""
    o, trees, flat, X, y, w, yhat, rok = problem(T, n, ARITH, 400, 82)
    out = {}
    for t in range(flat.ntrees):
        k, ar, c = flat.tree(t)
        if len(c) == 0 or not rok[t]:
            continue
        with np.errstate(all="ignore"):
            yh, gc, okt = oracle.eval_grad_consts(k, ar, c.astype(T), X, len(c), dtype=T)
        assert okt and np.array_equal(yh, yhat[t])
        out[t] = gc.astype(np.float64)
    return out


def margin_seed(loss, a, y):
    """dℓ/dŷ = y·L'(a) in float64."""
    return y.astype(np.float64) * M.deriv(loss.kind, loss.param, a).astype(np.float64)


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("loss", LOSSES, ids=lambda l: NAME[l.kind])
def test_gradients_match_the_reference(gpu_ctx, T, loss):
    """srhip_eval_loss_grad in the forward-mode interpreter (margin losses have no gradient
    tree code: last_tree_code is 0): every constant's Σ w·y·L'(a)·∂ŷ/∂c against the oracle's
    ∂ŷ/∂c in T, within rtol·Σ|terms| plus what a 4-ulp move of a does to L' (which covers
    the kinks), the bound of tests/test_jit_losses_gpu.py. ZeroOne's gradient is exactly 0."""
    n = 3001
    o, trees, flat, X, y, w, yhat, rok = problem(T, n, ARITH, 400, 82)
    ctx = gpu_ctx
    rtol, eps = RTOL[np.dtype(T)], float(np.finfo(T).eps)
    for weights in (None, w):
        ds = srhip.DeviceDataset(ctx, X, y, weights)
        prog = srhip.Program(ctx, flat, T)
        s, g, wsum, ok = prog.eval_loss_grad(ds, loss.kind, loss.params)
        assert ctx.last_tree_code() == 0
        ok = np.asarray(ok).astype(bool)
        assert np.array_equal(ok, rok)
        ref, mag = reference_sums(loss, yhat, y, weights)
        check_sums(s, ref, mag, wsum, ok, T, f"grad loss {NAME[loss.kind]} {np.dtype(T).name}")
        w64 = np.ones(n) if weights is None else weights.astype(np.float64)
        checked = 0
        for t, gc in const_grads(T, n).items():
            lo, hi = flat.const_off[t], flat.const_off[t + 1]
            with np.errstate(all="ignore"):
                a = yhat[t] * y  # in T
                seed = margin_seed(loss, a, y)
                term = w64 * seed * gc
                d = (4 * eps * np.abs(a.astype(np.float64))).astype(T)
                dv = np.maximum(np.abs(margin_seed(loss, a + d, y) - seed),
                                np.abs(margin_seed(loss, a - d, y) - seed)) * np.abs(w64 * gc)
            S, G, DV = np.abs(term).sum(axis=1), term.sum(axis=1), dv.sum(axis=1)
            sel = np.isfinite(S) & (S < 1e20)
            with np.errstate(invalid="ignore"):
                err = np.abs(g[lo:hi] - G)
            bound = rtol * S + DV + 1e-30
            assert np.all(err[sel] <= bound[sel]), (NAME[loss.kind], t, err[sel].tolist(), bound[sel].tolist())
            nonfin = ~np.isfinite(G)
            assert not np.isfinite(g[lo:hi][~sel & nonfin]).any(), (NAME[loss.kind], t)
            if loss.kind == K.LOSS["ZEROONE"]:
                assert not g[lo:hi].any(), t
            checked += int(sel.sum())
        assert checked > 300, checked


def test_constant_optimisation_decreases_a_margin_loss(gpu_ctx):
    """optimize_constants_batch with L2MarginLoss on 20 arithmetic trees that have
    constants: no returned loss exceeds the tree's starting loss, and some decrease."""
    T, n = np.float32, 3000
    _, trees, flat, X, y, w, yhat, rok = problem(T, n)
    o = srhip.Options(binary_operators=list(ARITH[0]), unary_operators=[], elementwise_loss=srhip.L2MarginLoss())
    picked = [t.copy() for t, k in zip(trees, rok) if k and srhip.has_constants(t)][:20]
    assert len(picked) == 20
    ds = srhip.Dataset(X, y)
    start, ok = srhip.eval_loss_batch_ok(picked, ds, o)
    assert ok.all()
    res = srhip.optimize_constants_batch(ds, picked, o, rng=np.random.default_rng(15))
    got = np.asarray(res.losses).astype(T)  # both in T, as eval_loss_batch_ok returns them
    assert np.all(got <= start), (got, start)
    assert np.any(got < start)
    after, ok = srhip.eval_loss_batch_ok(picked, ds, o)  # the trees were updated in place
    assert ok.all() and np.all(after <= start)


def test_parameter_rules(gpu_ctx):
    """check_loss: γ <= 0 and q <= 0 are invalid arguments; a q that is not integral is
    Unsupported (the reference's DomainError case stays with the CPU path)."""
    T, n = np.float32, 256
    o, trees, flat, X, y, w, yhat, rok = problem(T, n)
    prog = srhip.Program(gpu_ctx, flat, T)
    ds = srhip.DeviceDataset(gpu_ctx, X, y)
    for bad in (srhip.SmoothedL1HingeLoss(0.0), srhip.SmoothedL1HingeLoss(-0.5), srhip.DWDMarginLoss(0.0),
                srhip.DWDMarginLoss(-1.0)):
        for call in (prog.eval_loss, prog.eval_loss_grad):
            with pytest.raises(srhip.SrhipError) as e:
                call(ds, bad.kind, bad.params)
            assert e.value.code == _lib.ERR_INVALID and not isinstance(e.value, srhip.Unsupported)
    for call in (prog.eval_loss, prog.eval_loss_grad):
        with pytest.raises(srhip.Unsupported):
            call(ds, K.LOSS["DWDMARGIN"], [1.5])
    s, _, ok = prog.eval_loss(ds, K.LOSS["DWDMARGIN"], [2.0])  # an integral q runs
    assert np.asarray(ok).astype(bool).sum() == 197
    with pytest.raises(srhip.Unsupported):
        prog.eval_loss(ds, len(K.LOSSES), None)  # beyond the table
