"""Expression losses on the GPU: a custom elementwise loss written as an engine tree over
(prediction, target, weight), run by the loss-program interpreter in the tile epilogue of the
interpreter kernels (their own kernel mode) and, in dual numbers, by the gradient kernels.

The checker is the oracle applied twice (tests/expr_loss_cases.py): ŷ of the `+ - * /`
candidate trees is bit-exact by the project's own bar, the loss expression is evaluated by
the oracle over the rows (ŷ_t, y, w) in T, and the rows are summed in float64. The bound on
every succeeding tree is

    |got - ref| <= rtol·Σ|ℓ| + 4·eps(T)·n,   rtol = 1e-5 (Float32), 1e-9 (Float64)

(check_sums of tests/test_margin_losses_gpu.py with Σ|ℓ| as the magnitude and n as the
weight sum). The engine never multiplies by w: an expression that wants weights reads x3.
"""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine opens the device: the process then holds one HIP runtime)

import expr_loss_cases as E
import oracle
import srhip
from srhip import _lib
from srhip import constants as K
from test_margin_losses_gpu import RTOL, check_sums, program

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]


@functools.lru_cache(maxsize=None)
def reference(name, T, n, weighted, extra_deep=True, ntrees=200, seed=11):
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, n, ntrees, seed, extra_deep)
    ref, mag = E.reference_sums(name, yhat, y, w if weighted else None, rok, T)
    ref.setflags(write=False)
    mag.setflags(write=False)
    return ref, mag


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("n", [1, 256, 513, 3000])
def test_parity_with_the_oracle(gpu_ctx, n, T, weighted):
    """E1-E4 (E3 on the weighted dataset only) on problem A plus the six deep trees of
    tests/test_variant_matrix_gpu.py, so that both the shallow and the deep kernel variant run:
    n = 1 (a lone partial tile), 256, 513 (an interpreter tile of 512 and one row), 3000 (many
    tiles, the last partial). did_succeed is the candidate tree's alone, 197 of the 200 trees of
    problem A; every sum is within the bound; the call is fully interpreted, also for a program
    built with SRHIP_JIT=1 (tree code for every size)."""
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, n, extra_deep=True)
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, y, w if weighted else None)
    for jit in (None, "1"):
        prog = program(ctx, flat, T, jit)
        info = prog.pass_info()
        assert info["shallow"] > 0 and info["deep"] > 0, info
        for name in ("E1", "E2", "E3", "E4"):
            if name in E.USES_W and not weighted:
                continue
            loss = E.expr_loss(name)
            s, wsum, ok = prog.eval_loss(ds, loss.kind, loss.params)
            what = f"{name} {np.dtype(T).name} n={n} weighted={weighted} jit={jit}"
            assert ctx.last_tree_code() == 0, what
            ok = np.asarray(ok).astype(bool)
            assert np.array_equal(ok, rok), what
            assert int(ok[:200].sum()) == 197, what
            assert wsum == pytest.approx(float(w.astype(np.float64).sum() if weighted else n), rel=1e-6)
            ref, mag = reference(name, T, n, weighted)
            assert np.isfinite(ref[rok]).all(), what  # E1-E4 are finite on every succeeding tree
            nfin = check_sums(s, ref, mag, float(n), ok, T, what)
            assert nfin == int(rok.sum())


@pytest.mark.parametrize("T", DTYPES)
def test_equivalence_with_the_built_in_losses(gpu_ctx, T):
    """square(p - t), w·square(p - t) and abs(p - t) against the built-in L2, weighted L2 and
    unweighted L1 of the same interpreted program (SRHIP_JIT=0): identical did_succeed, sums
    within 1e-5·Σ|ℓ| (ℓ >= 0: Σ|ℓ| is the built-in's own sum)."""
    n = 3000
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, n, extra_deep=True)
    ctx = gpu_ctx
    prog = program(ctx, flat, T, "0")
    plain, weighted = srhip.DeviceDataset(ctx, X, y), srhip.DeviceDataset(ctx, X, y, w)
    for name, builtin, ds in (("SQ", srhip.L2DistLoss(), plain), ("WSQ", srhip.L2DistLoss(), weighted),
                              ("ABS", srhip.L1DistLoss(), plain)):
        sb, wb, okb = prog.eval_loss(ds, builtin.kind, builtin.params)
        assert ctx.last_tree_code() == 0
        loss = E.expr_loss(name)
        se, we, oke = prog.eval_loss(ds, loss.kind, loss.params)
        assert ctx.last_tree_code() == 0
        okb, oke = np.asarray(okb).astype(bool), np.asarray(oke).astype(bool)
        assert np.array_equal(okb, oke) and np.array_equal(oke, rok), name
        assert we == wb
        fin = oke & np.isfinite(sb)
        assert fin.sum() >= 190 and np.isfinite(se[fin]).all(), name
        err = np.abs(se[fin] - sb[fin])
        print(f"{name} {np.dtype(T).name}: worst err/Σ|ℓ| {float(np.max(err / sb[fin])):.3g}")
        assert np.all(err <= 1e-5 * sb[fin]), (name, np.flatnonzero(fin)[~(err <= 1e-5 * sb[fin])][:10])


@pytest.mark.parametrize("T", DTYPES)
def test_weight_contract(gpu_ctx, T):
    """The engine does not multiply by w: on a weighted dataset square(p - t) gives the
    unweighted Σ r² while out_weight_sum is Σ w; an expression that reads the weight is an
    invalid argument on an unweighted dataset, through every entry point that takes a loss."""
    n = 3000
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, n, extra_deep=True)
    ctx = gpu_ctx
    prog = srhip.Program(ctx, flat, T)
    loss = E.expr_loss("SQ")
    s, wsum, ok = prog.eval_loss(srhip.DeviceDataset(ctx, X, y, w), loss.kind, loss.params)
    ok = np.asarray(ok).astype(bool)
    assert np.array_equal(ok, rok)
    assert wsum == pytest.approx(float(w.astype(np.float64).sum()), rel=1e-6)
    ref, mag = reference("SQ", T, n, False)  # the unweighted sums
    check_sums(s, ref, mag, float(n), ok, T, f"SQ on a weighted dataset {np.dtype(T).name}")
    # which the weighted ones are far from (the median tree's differ by 23 %): the bound tells them apart
    refw, _ = reference("WSQ", T, n, True)
    assert np.median(np.abs(ref[rok] - refw[rok]) / mag[rok]) > 0.1
    e3 = E.expr_loss("E3")
    plain = srhip.DeviceDataset(ctx, X, y)
    rows = np.zeros((flat.ntrees, 4), dtype=np.int64)
    for call in (lambda: prog.eval_loss(plain, e3.kind, e3.params),
                 lambda: prog.eval_loss_grad(plain, e3.kind, e3.params),
                 lambda: prog.eval_loss_rowsets(plain, e3.kind, rows, e3.params)):
        with pytest.raises(srhip.SrhipError) as err:
            call()
        assert err.value.code == _lib.ERR_INVALID and not isinstance(err.value, srhip.Unsupported)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("T", DTYPES)
def test_a_non_finite_loss_does_not_fail_the_tree(gpu_ctx, T, weighted):
    """E5 = square(log(p / t)) is NaN wherever p and t differ in sign. At n = 513 every succeeding
    tree has such a row: ok is still the candidate tree's (197 succeed) and every sum is non-finite.
    At n = 1 the oracle finds 83 trees with a finite loss: those meet the bound, the others are
    non-finite."""
    ctx = gpu_ctx
    loss = E.expr_loss("E5")
    for n, nfinite in ((513, 0), (1, 83)):
        o, trees, flat, X, y, w, yhat, rok = E.problem(T, n)
        prog = srhip.Program(ctx, flat, T)
        s, wsum, ok = prog.eval_loss(srhip.DeviceDataset(ctx, X, y, w if weighted else None), loss.kind, loss.params)
        ok = np.asarray(ok).astype(bool)
        assert np.array_equal(ok, rok) and int(ok.sum()) == 197
        ref, mag = reference("E5", T, n, weighted, extra_deep=False)
        fin = rok & np.isfinite(ref)
        assert int(fin.sum()) == nfinite
        assert not np.isfinite(s[rok & ~fin]).any()
        check_sums(s, ref, mag, float(n), fin, T, f"E5 {np.dtype(T).name} n={n}")
        assert np.isnan(s[~rok]).all()  # a failed tree's sum is NaN as for every loss


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("name", ["E1", "E3"])
def test_per_tree_minibatches(gpu_ctx, T, name):
    """srhip_eval_loss_rowsets (the a.seg launch of the same kernel mode): 50 trees, each on its
    own sample of 50 rows drawn with replacement, one sample a single row repeated; the bound of
    this module per tree on its own sample. E3 needs weights; E1 runs weighted and not."""
    n, bs = 3000, 50
    o, trees, flat, X, y, w, _, _ = E.problem(T, n)
    sub = srhip.flatten(trees[:50], o, dtype=T)
    rng = np.random.default_rng(14)
    rows = rng.integers(0, n, (sub.ntrees, bs))
    rows[0, :] = rows[0, 0]
    rows[1, : bs // 2] = rows[1, bs // 2:]
    assert any(len(set(r)) < bs for r in rows[2:])
    with np.errstate(all="ignore"):
        per_tree = [oracle.eval_tree(*sub.tree(t), X[:, rows[t]], dtype=T) for t in range(sub.ntrees)]
    rok = np.array([p[1] for p in per_tree], dtype=bool)
    loss = E.expr_loss(name)
    eps = float(np.finfo(T).eps)
    for weights in ((w,) if name in E.USES_W else (None, w)):
        ds = srhip.Dataset(X, y, weights=weights)
        dev = ds.device()
        prog = srhip.engine.Program(dev.ctx, sub, T)
        s, ws, ok = prog.eval_loss_rowsets(dev, loss.kind, rows, loss.params)
        assert dev.ctx.last_tree_code() == 0
        assert np.array_equal(np.asarray(ok).astype(bool), rok)
        wsum = np.full(sub.ntrees, float(bs)) if weights is None else weights[rows].astype(np.float64).sum(axis=1)
        assert np.allclose(ws, wsum, rtol=1e-6)
        nchecked = 0
        for t in np.flatnonzero(rok):
            lr, fin = E.loss_rows(name, per_tree[t][0], y[rows[t]], None if weights is None else weights[rows[t]], T)
            assert fin, (name, t)
            ref, mag = lr.astype(np.float64).sum(), np.abs(lr.astype(np.float64)).sum()
            assert abs(s[t] - ref) <= RTOL[np.dtype(T)] * mag + 4 * eps * bs, (name, t, s[t], ref)
            nchecked += 1
        assert nchecked >= 30


def test_packed_partials_equal_eval_loss(gpu_ctx):
    """srhip_eval_loss_packed with E1 writes exactly pack_partials(srhip_eval_loss(...))."""
    from srhip.distributed import pack_partials

    T, n = np.float32, 3000
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, n, extra_deep=True)
    ctx = gpu_ctx
    loss = E.expr_loss("E1")
    for weights in (None, w):
        ds = srhip.DeviceDataset(ctx, X, y, weights)
        prog = srhip.Program(ctx, flat, T)
        buf = torch.full((2 * flat.ntrees + 1,), -7.0, dtype=torch.float64, device=f"cuda:{ctx.device}")
        prog.eval_loss_packed(ds, loss.kind, buf.data_ptr(), loss.params)
        ctx.sync()
        s, ws, ok = prog.eval_loss(ds, loss.kind, loss.params)
        assert not np.asarray(ok).astype(bool).all() and np.asarray(ok).astype(bool).sum() >= 197
        np.testing.assert_array_equal(buf.cpu().numpy(), pack_partials(s, ws, ok))


def seed_e1(r, y, w):
    return 2.5 * np.abs(r) ** 1.5 * np.sign(r)


def seed_e2(r, y, w):
    return 2 * r / (np.abs(y) + 1)


def seed_e3(r, y, w):
    return 2 * w * r / (1 + r * r)


def seed_e4(r, y, w):
    return np.tanh(r) + r / np.cosh(r) ** 2


SEEDS = {"E1": seed_e1, "E2": seed_e2, "E3": seed_e3, "E4": seed_e4}


@functools.lru_cache(maxsize=None)
def const_grads(T, n):
    """The oracle's ∂ŷ/∂c in T (as float64) of every succeeding tree of the gradient problem
    that has constants: {tree: [nconst, n]}, computed once per dtype."""
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, n, 400, 82)
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


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("name", ["E1", "E2", "E3", "E4"])
def test_gradients_match_the_reference(gpu_ctx, T, name):
    """srhip_eval_loss_grad: the loss program in dual numbers seeds every constant's
    Σ (dℓ/dŷ)·∂ŷ/∂c (no implicit w), fully interpreted. Against the oracle's ∂ŷ/∂c in T times the
    analytic seed written in NumPy float64 at the T-valued r = ŷ - y, within rtol·Σ|terms| plus what
    a 4-ulp move of r does to the seed (the bound of test_margin_losses_gpu's gradient test). E4 uses
    the prediction twice: both uses carry the tangent.

    The problem (400 trees, seed 82, n = 3001) from the oracle alone, the same in both dtypes:
    397 trees succeed and E1-E4 are finite on all of them; 381 of them have constants, 1707
    constants in all; a finite Σ|terms| below 1e20, hence a check, have 1679 of them under E1, 1698
    under E2 and all 1707 under E3 and E4 (at least 300 must be checked)."""
    n = 3001
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, n, 400, 82)
    ctx = gpu_ctx
    rtol, eps = RTOL[np.dtype(T)], float(np.finfo(T).eps)
    loss = E.expr_loss(name)
    seed_fn = SEEDS[name]
    y64, w64 = y.astype(np.float64), w.astype(np.float64)
    for weighted in ((True,) if name in E.USES_W else (False, True)):
        ds = srhip.DeviceDataset(ctx, X, y, w if weighted else None)
        prog = srhip.Program(ctx, flat, T)
        s, g, wsum, ok = prog.eval_loss_grad(ds, loss.kind, loss.params)
        assert ctx.last_tree_code() == 0
        ok = np.asarray(ok).astype(bool)
        assert np.array_equal(ok, rok)
        ref, mag = reference(name, T, n, weighted, extra_deep=False, ntrees=400, seed=82)
        check_sums(s, ref, mag, float(n), ok & np.isfinite(ref), T, f"grad loss {name} {np.dtype(T).name}")
        checked = 0
        for t, gc in const_grads(T, n).items():
            lo, hi = flat.const_off[t], flat.const_off[t + 1]
            with np.errstate(all="ignore"):
                r = yhat[t] - y  # in T
                r64 = r.astype(np.float64)
                seed = seed_fn(r64, y64, w64)
                term = seed * gc
                d = (4 * eps * np.abs(r64)).astype(T).astype(np.float64)
                dv = np.maximum(np.abs(seed_fn(r64 + d, y64, w64) - seed),
                                np.abs(seed_fn(r64 - d, y64, w64) - seed)) * np.abs(gc)
            S, G, DV = np.abs(term).sum(axis=1), term.sum(axis=1), dv.sum(axis=1)
            sel = np.isfinite(S) & (S < 1e20)
            with np.errstate(invalid="ignore"):
                err = np.abs(g[lo:hi] - G)
            bound = rtol * S + DV + 1e-30
            assert np.all(err[sel] <= bound[sel]), (name, t, err[sel].tolist(), bound[sel].tolist())
            checked += int(sel.sum())
        assert checked >= 300, checked


def test_constant_optimisation_decreases_an_expression_loss(gpu_ctx):
    """optimize_constants_batch with E2 on 20 succeeding trees that have constants: no returned
    loss exceeds the tree's starting loss, and some decrease."""
    T, n = np.float32, 3000
    _, trees, flat, X, y, w, yhat, rok = E.problem(T, n)
    o = srhip.Options(binary_operators=list(E.ARITH), unary_operators=[], elementwise_loss=E.expr_loss("E2"))
    picked = [t.copy() for t, k in zip(trees, rok) if k and srhip.has_constants(t)][:20]
    assert len(picked) == 20
    ds = srhip.Dataset(X, y)
    start, ok = srhip.eval_loss_batch_ok(picked, ds, o)
    assert ok.all()
    res = srhip.optimize_constants_batch(ds, picked, o, rng=np.random.default_rng(15))
    got = np.asarray(res.losses).astype(T)
    assert np.all(got <= start), (got, start)
    assert np.any(got < start)
    after, ok = srhip.eval_loss_batch_ok(picked, ds, o)  # the trees were updated in place
    assert ok.all() and np.all(after <= start)


def test_handle_lifetime(gpu_ctx):
    """Two handles alive at once give their own results; evaluating with a destroyed handle is an
    invalid argument (also after the context has run it), and the other handle still works."""
    T, n = np.float32, 513
    o, trees, flat, X, y, w, yhat, rok = E.problem(T, n, extra_deep=True)
    ctx = gpu_ctx
    lo = E.loss_options()
    a, b = srhip.ExprLoss(E.e1(lo), lo), srhip.ExprLoss(E.absr(lo), lo)
    assert a.kind != b.kind
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = srhip.Program(ctx, flat, T)
    for _ in range(2):  # interleaved: each keeps its own program on the device
        for loss, name in ((a, "E1"), (b, "ABS")):
            s, _, ok = prog.eval_loss(ds, loss.kind, loss.params)
            ref, mag = reference(name, T, n, False)
            check_sums(s, ref, mag, float(n), np.asarray(ok).astype(bool), T, f"lifetime {name}")
    a.destroy()
    for call in (prog.eval_loss, prog.eval_loss_grad):
        with pytest.raises(srhip.SrhipError) as err:
            call(ds, a.kind, None)
        assert err.value.code == _lib.ERR_INVALID and not isinstance(err.value, srhip.Unsupported)
    s, _, ok = prog.eval_loss(ds, b.kind, None)
    ref, mag = reference("ABS", T, n, False)
    check_sums(s, ref, mag, float(n), np.asarray(ok).astype(bool), T, "lifetime ABS after destroy")
    with pytest.raises(srhip.SrhipError) as err:  # never registered
        prog.eval_loss(ds, K.EXPR_LOSS_BEGIN + 10**6, None)
    assert err.value.code == _lib.ERR_INVALID
    with pytest.raises(srhip.Unsupported):  # between the table and the handles: still unsupported
        prog.eval_loss(ds, len(K.LOSSES), None)
