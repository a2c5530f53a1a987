"""Wide datasets on the GPU: feature counts whose row tile of all features does not fit in
LDS (79 or more features for the shallow interpreters, 159 or more for every kernel) run in the
wide interpreter kernels, which read their feature operands from global memory
(DESIGN.md §3.14). On the parent of this feature these calls raise srhip.Unsupported.

The inputs are tests/wide_cases.py's. Checked on the CPU with the oracle: of the 200 random
trees 164-165 (Float32) and 181 (Float64) succeed with a finite loss at 80, 160 and 300
features and 700 rows, so every parity case compares at least 150 trees. Bars: did_succeed
equal to the oracle's on every tree; losses within 1e-5 relative (1e-9 for the Float64 checks
that other GPU tests hold to 1e-9) beyond the conditioned spread of tests/numerics.py, used as
tests/test_gpu_parity.py uses it; per-row outputs of the wide and the LDS kernels bit for bit.
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine opens the device: the process then holds one HIP runtime)

import expr_loss_cases as EL
import expr_op_cases as EO
import oracle
import srhip
import wide_cases as W
from numerics import assert_close_conditioned, loss_spread
from srhip import Node
from srhip.interface import _seed_features
from test_gradients import grad_spread, oracle_grad
from test_margin_losses_gpu import check_sums, reference_sums

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
L2 = 0  # SRHIP_LOSS_L2 (include/srhip.h)


class wide_env:
    """SRHIP_WIDE set (or unset: None) for a block; the engine reads it per call."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("SRHIP_WIDE")
        if self.value is None:
            os.environ.pop("SRHIP_WIDE", None)
        else:
            os.environ["SRHIP_WIDE"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("SRHIP_WIDE", None)
        else:
            os.environ["SRHIP_WIDE"] = self.old


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check_l2_parity(ctx, T, nfeat, n, ntrees, weighted, min_compared, what):
    o, trees, flat, X, y, w = W.problem(T, nfeat, n, ntrees)
    ds = srhip.Dataset(X, y, weights=w if weighted else None)
    losses, ok = srhip.eval_loss_batch_ok(trees, ds, o)
    name = ctx.last_kernel_name()
    ref, rok, spread = W.reference(T, nfeat, n, ntrees, weighted)
    assert "wide" in name, (what, name)
    assert np.array_equal(ok, rok), (what, np.flatnonzero(ok != rok))
    assert not ok[-1], what  # exp(exp(exp(50·x_nfeat))) overflows
    m = ok & np.isfinite(ref)
    with np.errstate(all="ignore"):
        rel = np.abs(losses[m].astype(np.float64) - ref[m]) / np.abs(ref[m])
    print(f"{what}: {int(m.sum())} trees compared, max rel {float(np.nanmax(rel)):.3g}, kernel {name}")
    assert m.sum() >= min_compared, (what, int(m.sum()))
    assert m[-6:-1].all(), what  # the hand-made trees reading x_nfeat are among them
    assert_close_conditioned(losses[m], ref[m], spread[m], rtol=1e-5, msg=what)
    assert np.all(np.isinf(losses[~ok]))


# ---- 1. loss parity -------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("nfeat", [80, 160, 300])
@pytest.mark.parametrize("T", DTYPES)
def test_l2_losses_match_the_oracle(gpu_ctx, T, nfeat, weighted):
    """80 features: past the shallow interpreters' 79 arrays; 160: past every LDS kernel;
    300: feature × n_pad well past the rows of one feature."""
    check_l2_parity(gpu_ctx, T, nfeat, 700, 200, weighted, 150,
                    f"L2 {np.dtype(T).name} nfeat={nfeat} weighted={weighted}")


# ---- 2. row-count edges ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65, 8200])
def test_row_count_edges(gpu_ctx, n):
    """One row, one full wave row, one past it, and 8200: past the 8192-row workgroup cap.
    (Fewer trees fail on few rows; at 8200 rows 150 of the 200 still have a finite loss.)"""
    check_l2_parity(gpu_ctx, np.float32, 160, n, 200, False, 150, f"L2 f32 nfeat=160 n={n}")


# ---- 3. per-row outputs, bit for bit --------------------------------------------------------
def outputs_and_sums(ctx, flat, T, X, y):
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = srhip.Program(ctx, flat, T)
    out, ok = prog.eval_tree_array(ds)
    kout = ctx.last_kernel_name()
    s, _, lok = prog.eval_loss(ds, L2)
    return out, np.asarray(ok).astype(bool), kout, s, np.asarray(lok).astype(bool), ctx.last_kernel_name()


def assert_same_outputs(a, b, T, what):
    out_a, ok_a, _, s_a, lok_a, _ = a
    out_b, ok_b, _, s_b, lok_b, _ = b
    assert np.array_equal(ok_a, ok_b) and np.array_equal(lok_a, lok_b) and np.array_equal(ok_a, lok_a), what
    assert ok_a.sum() >= 150 and not ok_a.all(), what
    # the rows of a succeeding tree bit for bit; a failed tree's rows are not defined by the
    # reference: equal up to the payload of a NaN
    assert np.array_equal(bits(out_a[ok_a]), bits(out_b[ok_a])), what
    assert np.array_equal(out_a[~ok_a], out_b[~ok_a], equal_nan=True), what
    # the tile size differs, so the summation order does: 1e-5 only (ℓ >= 0: Σ|ℓ| is the sum)
    fin = lok_a & np.isfinite(s_a)
    assert np.array_equal(fin, lok_b & np.isfinite(s_b)), what
    err = np.abs(s_a[fin] - s_b[fin])
    print(f"{what}: {int(ok_a.sum())} trees bitwise equal, worst sum difference {float(np.max(err / s_a[fin])):.3g}")
    assert np.all(err <= 1e-5 * s_a[fin]), what


@pytest.mark.parametrize("T", DTYPES)
def test_per_row_outputs_equal_the_lds_kernels_bit_for_bit(gpu_ctx, T):
    """Trees that read features 1..20 only, on X[:20] (the LDS kernels) and on the whole
    160-feature X (the wide kernels)."""
    o, trees, flat, X, y, w = W.problem(T, 160, read=20)
    narrow = outputs_and_sums(gpu_ctx, flat, T, np.ascontiguousarray(X[:20]), y)
    wide = outputs_and_sums(gpu_ctx, flat, T, X, y)
    assert "wide" not in narrow[2] and "wide" not in narrow[5], narrow[2]
    assert "wide" in wide[2] and "wide" in wide[5], wide[2]
    assert_same_outputs(narrow, wide, T, f"X[:20] against 160 features, {np.dtype(T).name}")


@pytest.mark.parametrize("T", DTYPES)
def test_forced_wide_equals_the_lds_kernels_bit_for_bit(gpu_ctx, T):
    """Five features, where the default is the LDS kernels: SRHIP_WIDE=1 against unset."""
    o, trees, flat, X, y, w = W.problem(T, 5)
    with wide_env(None):
        narrow = outputs_and_sums(gpu_ctx, flat, T, X, y)
    with wide_env("1"):
        wide = outputs_and_sums(gpu_ctx, flat, T, X, y)
    assert "wide" not in narrow[2] and "wide" not in narrow[5], narrow[2]
    assert "wide" in wide[2] and "wide" in wide[5], wide[2]
    assert_same_outputs(narrow, wide, T, f"SRHIP_WIDE=1 against unset, {np.dtype(T).name}")


# ---- 4. the other loss families -------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("T", DTYPES)
def test_huber_loss(gpu_ctx, T, weighted):
    """The generic loss tail, against the oracle as tests/test_gpu_parity.py
    test_weighted_and_all_losses checks it (1e-9 there in Float64)."""
    loss = srhip.HuberLoss(0.8)
    o, trees, flat, X, y, w = W.problem(T, 160)
    lo = srhip.Options(binary_operators=list(W.OPS[0]), unary_operators=list(W.OPS[1]), elementwise_loss=loss)
    l, ok = srhip.eval_loss_batch_ok(trees, srhip.Dataset(X, y, weights=w if weighted else None), lo)
    assert "wide" in gpu_ctx.last_kernel_name()
    ref, rok, spread = W.reference(T, 160, weighted=weighted, loss=loss)
    assert np.array_equal(ok, rok)
    m = ok & np.isfinite(ref)
    assert m.sum() >= 150
    assert_close_conditioned(l[m], ref[m], spread[m], rtol=1e-5 if T == np.float32 else 1e-9, msg="Huber")


@pytest.mark.parametrize("T", DTYPES)
def test_margin_loss(gpu_ctx, T):
    """L1Hinge on y ∈ {−1, +1}, + − × ÷ trees: tests/test_margin_losses_gpu.py's checker and bound."""
    loss = srhip.L1HingeLoss()
    o, trees, flat, X, y, w = W.problem(T, 160, ops=W.ARITH, classes=True)
    yhat, rok = W.predictions(T, 160, classes=True)
    ctx = gpu_ctx
    prog = srhip.Program(ctx, flat, T)
    for weights in (None, w):
        s, wsum, ok = prog.eval_loss(srhip.DeviceDataset(ctx, X, y, weights), loss.kind, loss.params)
        assert "wide" in ctx.last_kernel_name()
        ok = np.asarray(ok).astype(bool)
        assert np.array_equal(ok, rok)
        ref, mag = reference_sums(loss, yhat, y, weights)
        nfin = check_sums(s, ref, mag, wsum, ok, T, f"L1Hinge {np.dtype(T).name} weighted={weights is not None}")
        assert nfin >= 150


@pytest.mark.parametrize("T", DTYPES)
def test_expression_loss(gpu_ctx, T):
    """E2 and, weighted, E3 of tests/expr_loss_cases.py: the checker and bound of
    tests/test_expr_loss_gpu.py."""
    o, trees, flat, X, y, w = W.problem(T, 160, ops=W.ARITH)
    yhat, rok = W.predictions(T, 160)
    ctx = gpu_ctx
    prog = srhip.Program(ctx, flat, T)
    for name, weights in (("E2", None), ("E3", w)):
        loss = EL.expr_loss(name)
        s, wsum, ok = prog.eval_loss(srhip.DeviceDataset(ctx, X, y, weights), loss.kind, loss.params)
        assert "wide" in ctx.last_kernel_name() and ctx.last_tree_code() == 0
        ok = np.asarray(ok).astype(bool)
        assert np.array_equal(ok, rok)
        ref, mag = EL.reference_sums(name, yhat, y, weights, rok, T)
        assert np.isfinite(ref[rok]).all()
        nfin = check_sums(s, ref, mag, float(len(y)), ok, T, f"{name} {np.dtype(T).name}")
        assert nfin == int(rok.sum()) and nfin >= 150


# ---- 5. minibatches ------------------------------------------------------------------------
@pytest.mark.parametrize("T", DTYPES)
def test_shared_row_idx_with_repeated_indices(gpu_ctx, T):
    o, trees, flat, X, y, w = W.problem(T, 160)
    idx = np.random.default_rng(24).integers(0, 700, 300)
    idx[:40] = idx[40:80]  # repeated indices
    for weights in (None, w):
        l, ok = srhip.eval_loss_batch_ok(trees, srhip.Dataset(X, y, weights=weights), o, row_idx=idx)
        assert "wide" in gpu_ctx.last_kernel_name()
        with np.errstate(all="ignore"):
            _, rl, rok = oracle.eval_loss_batch(flat, X, y, weights, row_idx=idx, dtype=T)
        assert np.array_equal(ok, rok)
        m = ok & np.isfinite(rl)
        assert m.sum() >= 150
        wv = None if weights is None else weights[idx]
        sp = loss_spread(trees, o, X[:, idx], y[idx], wv, T) / (len(idx) if wv is None else wv.sum())
        assert_close_conditioned(l[m], rl[m], sp[m], rtol=1e-5, msg="shared row_idx")


@pytest.mark.parametrize("T", DTYPES)
def test_per_tree_row_sets(gpu_ctx, T):
    """eval_loss_batch_rowsets, batch_size 50, weighted, against the oracle tree by tree
    (tests/test_rowsets_gpu.py's checker)."""
    from test_rowsets_gpu import oracle_rowsets, spread_rowsets

    o, trees, flat, X, y, w = W.problem(T, 160)
    trees = trees[:60] + trees[200:]
    rng = np.random.default_rng(41)
    rows = [rng.integers(0, 700, 50) for _ in trees]
    rows[0][:] = rows[0][0]  # one sample that is a single row repeated
    l, ok = srhip.eval_loss_batch_rowsets(trees, srhip.Dataset(X, y, weights=w), o, rows)
    assert "wide" in gpu_ctx.last_kernel_name()
    with np.errstate(all="ignore"):
        rl, rok = oracle_rowsets(trees, o, X, y, w, rows, T)
    assert np.array_equal(ok, rok)
    m = ok & np.isfinite(rl)
    assert m.sum() >= 45 and m[-6:-1].all()
    sp = spread_rowsets([t for t, k in zip(trees, m) if k], o, X, y, w, [r for r, k in zip(rows, m) if k], T)
    assert_close_conditioned(l[m], rl[m], sp, rtol=1e-5, msg="row sets")
    assert np.all(np.isinf(l[~ok]))


# ---- 6. gradients --------------------------------------------------------------------------
def constant_trees(o, trees, nfeat, limit=60):
    """The first `limit` random trees with constants and hand-made ones that read x_nfeat
    next to a constant: fused (c, x), (x, c) operands, a unary chain, six constants (two
    tangent groups), and a deep tree."""
    B, U = o.make_binary, o.make_unary
    last, c = (lambda: Node(feature=nfeat)), (lambda v: Node(val=v))
    hand = [B("*", c(1.5), last()), B("-", last(), c(0.25)), B("+", U("cos", B("*", c(0.7), last())), c(0.75)),
            B("+", B("+", B("*", c(0.1), last()), B("*", c(0.2), Node(feature=2))),
              B("*", B("+", c(0.3), B("*", c(0.4), last())), B("+", c(0.5), B("*", c(0.6), Node(feature=1))))),
            B("*", W.deep_tree(o, nfeat), c(0.5))]
    return [t for t in trees[:200] if srhip.has_constants(t)][:limit] + hand


@pytest.mark.parametrize("force", [None, "1"], ids=["default", "SRHIP_WIDE=1"])
@pytest.mark.parametrize("nfeat", [160, 300])
@pytest.mark.parametrize("T", DTYPES)
def test_loss_gradients_match_the_oracle(gpu_ctx, T, nfeat, force):
    """eval_loss_grad_batch (L2) against the oracle's forward mode with grad_spread, as
    tests/test_gradients.py uses it per row. Reference, per constant, in float64:
    g = mean_i 2·r_i·∂ŷ_i/∂c, r = ŷ − y. Bound: rtol·mean_i|2·r_i·∂ŷ_i/∂c| (the engine sums
    T-valued terms: rtol = 1e-5 Float32, 1e-9 Float64, the loss bars) + 4 × the spread that
    grad_spread's per-row spreads (sv of ŷ, sg of ∂ŷ/∂c) give the mean:
    mean_i 2·(|r_i|·sg_i + |∂ŷ_i/∂c|·sv_i + sv_i·sg_i).
    The gradient kernels' row tiles are smaller than the evaluation kernels': a 160- or
    300-feature tile fits some of them, so the default run is wide only in part;
    SRHIP_WIDE=1 runs every pass wide."""
    o, trees, flat, X, y, w = W.problem(T, nfeat)
    trees = constant_trees(o, trees, nfeat)
    with wide_env(force):
        losses, grads, ok = srhip.eval_loss_grad_batch(trees, srhip.Dataset(X, y), o)
        name = gpu_ctx.last_kernel_name()
        ref_l, ref_ok = srhip.eval_loss_batch_ok(trees, srhip.Dataset(X, y), o)
    if force == "1":
        assert "grad_kernel_wide" in name, name
    with np.errstate(all="ignore"):
        _, ok_T = oracle.eval_trees(srhip.flatten(trees, o, dtype=T), X, dtype=T)
    assert np.array_equal(ok, ok_T) and np.array_equal(ok, ref_ok)
    rtol = 1e-5 if T == np.float32 else 1e-9
    got, ref, spread, mag = [], [], [], []
    y64 = y.astype(np.float64)
    for t, tree in enumerate(trees):
        with np.errstate(all="ignore"):
            v0, g0, rok, sv, sg = grad_spread(tree, o, X, T)
            if not (ok[t] and rok):
                continue
            r = v0 - y64
            got.append(np.asarray(grads[t], dtype=np.float64))
            ref.append(np.mean(2 * r * g0, axis=1))
            mag.append(np.mean(np.abs(2 * r * g0), axis=1))
            spread.append(np.mean(2 * (np.abs(r) * sg + np.abs(g0) * sv + sv * sg), axis=1))
    cat = np.concatenate
    got, ref, spread, mag = cat(got), cat(ref), cat(spread), cat(mag)
    # the engine sums T-valued terms in T: constants whose Σ_i|2·r_i·∂ŷ_i/∂c| = n·mag comes
    # within 2^10 of T's largest number overflow there (9 of 218 in Float32 at 160 features:
    # references of 7e36..2e38) and are left out
    fin = np.isfinite(ref) & np.isfinite(mag) & (len(y) * mag < float(np.finfo(T).max) * 2.0 ** -10)
    print(f"loss gradients {np.dtype(T).name} nfeat={nfeat} {name}: {int(fin.sum())} constants checked")
    assert fin.sum() >= 60
    assert_close_conditioned(got[fin], ref[fin], spread[fin] + rtol * mag[fin] / 4, rtol=0.0, msg="dL/dc")
    m = ok & np.isfinite(ref_l)
    np.testing.assert_allclose(losses[m], ref_l[m], rtol=1e-5 if T == np.float32 else 1e-9)


@pytest.mark.parametrize("force", [None, "1"], ids=["default", "SRHIP_WIDE=1"])
def test_per_row_constant_gradients(gpu_ctx, force):
    """eval_grad_tree_array of three trees reading x_160, Float64, against the oracle's
    forward mode (the bars of tests/test_gradients.py test_many_constants_and_deep_trees)."""
    o, trees, flat, X, y, w = W.problem(np.float64, 160)
    three = constant_trees(o, trees, 160, limit=0)[2:]
    with wide_env(force):
        val, grads, ok = srhip.eval_grad_tree_array(three, X, o)
        name = gpu_ctx.last_kernel_name()
    if force == "1":
        assert "grad_kernel_wide" in name, name
    for t, tree in enumerate(three):
        rv, rg, rok = oracle_grad(tree, o, X)
        assert ok[t] and rok
        np.testing.assert_allclose(val[t], rv, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(grads[t], rg, rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("force", [None, "1"], ids=["default", "SRHIP_WIDE=1"])
def test_feature_gradients(gpu_ctx, force):
    """eval_grad_tree_array(variable=True) at 100 features, Float64, against the oracle's
    forward mode on the same seeded trees (tests/test_feature_gradients.py)."""
    nfeat, n = 100, 200
    o, trees, flat, X, y, w = W.problem(np.float64, nfeat, n, 40)
    trees = trees[:40] + trees[-6:-1]
    with wide_env(force):
        val, grads, ok = srhip.eval_grad_tree_array(trees, X, o, variable=True)
    plus = o.binary_operators.index("+") + 1
    got, ref, spread = [], [], []
    nchecked = 0
    for t, tree in enumerate(trees):
        aug, seeds = _seed_features(tree, plus, None)
        with np.errstate(all="ignore"):
            rv, rg, rok, sv, sg = grad_spread(aug, o, X, np.float64)
        assert bool(ok[t]) == bool(rok)
        if not ok[t]:
            continue
        seeds = np.asarray(seeds)
        assert grads[t].shape == (nfeat, n)
        for f in range(1, nfeat + 1):
            m = seeds == f
            got.append(grads[t][f - 1])
            ref.append(rg[m].sum(axis=0) if m.any() else np.zeros(n))
            spread.append(sg[m].sum(axis=0) if m.any() else np.zeros(n))
            nchecked += int(m.any())
    cat = np.concatenate
    assert_close_conditioned(cat(got), cat(ref), cat(spread), rtol=1e-11, atol=1e-11, msg="feature gradients")
    assert nchecked > 50
    assert np.any(grads[-5][nfeat - 1] != 0)  # x_nfeat's own gradient


# ---- 7. expression operators ---------------------------------------------------------------
@pytest.mark.parametrize("T", DTYPES)
def test_expression_operators(gpu_ctx, T):
    """custom_cos (unary) and my_func_a (binary) on x_160 against their expansions, bit for
    bit; nexp(x_160) = inv(exp(x_160)) where exp overflows succeeds (opaque semantics) while
    its expansion fails."""
    nfeat, n = 160, 700
    o = EO.options(("custom_cos", "my_func_a", "nexp"))
    po = EO.prim_options()
    U, B = o.make_unary, o.make_binary
    last, x1 = (lambda: Node(feature=nfeat)), (lambda: Node(feature=1))
    trees = [U("custom_cos", last()), B("my_func_a", last(), x1()),
             B("+", U("custom_cos", B("*", last(), Node(val=0.5))), B("my_func_a", x1(), U("cos", last()))),
             B("+", U("nexp", last()), Node(feature=2))]
    X = np.array(W.problem(T, nfeat)[3])
    big = T(100.0 if T == np.float32 else 1000.0)
    X[nfeat - 1, 7] = big
    y = np.zeros(n, dtype=T)
    flat = srhip.flatten(trees, o, dtype=T)
    xflat = srhip.flatten([EO.expand(t, o) for t in trees], po, dtype=T)
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, y)
    out, ok = srhip.Program(ctx, flat, T).eval_tree_array(ds)
    assert "wide" in ctx.last_kernel_name()
    xout, xok = srhip.Program(ctx, xflat, T).eval_tree_array(ds)
    assert "wide" in ctx.last_kernel_name()
    with np.errstate(all="ignore"):
        _, rok = oracle.eval_trees(xflat, X, dtype=T)
    assert np.array_equal(xok, rok)
    assert list(ok) == [True, True, True, True] and list(xok) == [True, True, True, False]
    for t in range(3):
        assert np.array_equal(bits(out[t]), bits(xout[t])), t
    assert out[3, 7] == X[1, 7]  # inv(exp(1000)) = 0 inside the body
    rows = np.arange(n) != 7
    assert np.array_equal(bits(out[3][rows]), bits(xout[3][rows]))
    _, _, lok = srhip.Program(ctx, flat, T).eval_loss(ds, L2)
    assert np.asarray(lok).astype(bool).all()


# ---- 8. above the tree-code bar ------------------------------------------------------------
@pytest.mark.parametrize("T", DTYPES)
def test_a_batch_above_the_tree_code_bar_runs_wide(gpu_ctx, T):
    """300 trees (tree code from 256): the tree code's tile does not fit either, the batch
    runs in the wide interpreter; the packed partials equal eval_loss's sums."""
    from srhip.distributed import pack_partials

    check_l2_parity(gpu_ctx, T, 160, 700, 300, False, 225, f"300 trees {np.dtype(T).name}")
    assert gpu_ctx.last_tree_code() == 0
    o, trees, flat, X, y, w = W.problem(T, 160, 700, 300)
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, y, w)
    prog = srhip.Program(ctx, flat, T)
    buf = torch.full((2 * flat.ntrees + 1,), -7.0, dtype=torch.float64, device=f"cuda:{ctx.device}")
    prog.eval_loss_packed(ds, L2, buf.data_ptr())
    ctx.sync()
    assert "wide" in ctx.last_kernel_name() and ctx.last_tree_code() == 0
    s, ws, ok = prog.eval_loss(ds, L2)
    assert ctx.last_tree_code() == 0
    np.testing.assert_array_equal(buf.cpu().numpy(), pack_partials(s, ws, ok))


# ---- 9. constant optimisation --------------------------------------------------------------
def test_constant_optimisation(gpu_ctx):
    """20 trees with constants at 160 features, BFGS: no returned loss above the loss at x0,
    and the oracle's loss at the returned constants within 1e-5 of the returned loss."""
    T = np.float32
    o, trees, flat, X, y, w = W.problem(T, 160)
    trees = [t.copy() for t in constant_trees(o, trees, 160, limit=15)]
    assert len(trees) == 20
    ds = srhip.Dataset(X, y)
    start, ok0 = srhip.eval_loss_batch_ok(trees, ds, o)
    assert "wide" in gpu_ctx.last_kernel_name()
    res = srhip.optimize_constants_batch(ds, trees, o, rng=np.random.default_rng(52))
    got = np.asarray(res.losses).astype(T)
    print("constant optimisation: start", start, "returned", got, "converged", res.converged)
    assert np.all(got[ok0] <= start[ok0]), (got, start)
    assert res.converged.any() and np.any(got[ok0] < start[ok0])
    with np.errstate(all="ignore"):
        _, rl, rok = oracle.eval_loss_batch(srhip.flatten(trees, o, dtype=T), X, y, dtype=T)  # updated in place
    fin = np.isfinite(got)
    assert np.array_equal(fin, rok & np.isfinite(rl))
    np.testing.assert_allclose(got[fin], rl[fin], rtol=1e-5)


# ---- 10. the switch ------------------------------------------------------------------------
@pytest.mark.parametrize("T", DTYPES)
def test_switch_off_is_unsupported_again(gpu_ctx, T):
    o, trees, flat, X, y, w = W.problem(T, 160)
    ds = srhip.Dataset(X, y)
    with wide_env("0"):
        with pytest.raises(srhip.Unsupported):
            srhip.eval_loss_batch_ok(trees, ds, o)
    losses, ok = srhip.eval_loss_batch_ok(trees, ds, o)  # and unset it runs
    assert ok.sum() >= 150


def test_the_deep_hand_made_tree_needs_the_deep_list(gpu_ctx):
    """The hand-made deep tree does need more than the shallow kernels' two stack slots."""
    o, trees, flat, X, y, w = W.problem(np.float32, 160)
    info = srhip.Program(gpu_ctx, srhip.flatten([W.deep_tree(o, 160)], o, dtype=np.float32), np.float32).pass_info()
    assert info["deep"] == 1 and info["shallow"] == 0, info
