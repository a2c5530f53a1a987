"""Multi-output datasets on the GPU: one X with K target columns (each with its own
weight column), scored through per-target views and through the fused calls that
give every tree of one launch its own target (srhip_eval_loss_targets,
srhip_eval_loss_rowsets_targets).

The reference value of tree t is always the oracle on (X, Y[target[t]], W[target[t]]),
one target at a time. Bars (those of tests/test_rowsets_gpu.py): did_succeed identical
on every tree; losses within 1e-5 relative (Float32; 1e-9 Float64) beyond the
conditioned perturbation spread of tests/numerics.py, no tree left out. The C oracle
has the distance losses only; for L1HingeLoss the reference is the project's margin
checker (tests/margin_reference.py) on the oracle's per-row predictions, and the
spread is Σ w·|y|·(the oracle's output spread): max(0, 1 - y·ŷ) moves by at most
|y|·|Δŷ|.

Checked on the CPU with the oracle: of the 159 trees 138 succeed in Float32 (137 with a
finite L2 loss) and 39 in Float64 (mixed-sign X under safe_log / safe_sqrt / ^), on all
rows and on rows 1000..2500 alike; every comparison needs 100 and 30 of them.

Shapes: 2500 rows (several row tiles with a partial last one at R = 8 and R = 4),
5 features, K = 3, 150 random trees plus nine deep ones (both interpreter passes).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import expr_loss_cases as EL
import margin_reference as M
import oracle
import srhip
import wide_cases as WC
from numerics import assert_close_conditioned, loss_spread, output_spread
from srhip import _lib
from srhip import constants as K
from test_rowsets_gpu import F32_OPS, NAN_OPS, deep_tree

pytestmark = pytest.mark.gpu

N, NFEAT, NT = 2500, 5, 3
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
RTOL = {np.float32: 1e-5, np.float64: 1e-9}
L2, HUBER, HINGE = srhip.L2DistLoss(), srhip.HuberLoss(1.0), srhip.L1HingeLoss()
LOSSES = [pytest.param(L2, id="L2"), pytest.param(HUBER, id="Huber"), pytest.param(HINGE, id="L1Hinge")]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def problem(T, n=N):
    """(options, trees, flat, X, Y, W): computed once per dtype, shared, never written to.
    Column 1 of Y is ±1 (the margin loss's classes)."""
    T = np.dtype(T).type
    ops = F32_OPS if T == np.float32 else NAN_OPS  # Float64: safe_log / safe_sqrt / ^ fail on some rows
    o = srhip.Options(binary_operators=ops[0], unary_operators=ops[1])
    rng = np.random.default_rng(141)
    trees = list(srhip.random_population(150, o, NFEAT, T, seed=142))
    trees += [deep_tree(d, rng) for d in (6, 7, 8) for _ in range(3)]  # the deep interpreter pass too
    if T == np.float32:
        X = rng.standard_normal((NFEAT, n)).astype(T)
    else:
        X = rng.uniform(-3, 3, (NFEAT, n))
    base = 2 * np.cos(X[3]) + X[0] * X[0] - 2
    Y = np.stack([base, np.where(base >= 0, 1, -1), X[1] * X[2] + 0.5]).astype(T)
    W = np.abs(rng.standard_normal((NT, n))).astype(T) + T(0.01)
    flat = srhip.flatten(trees, o, dtype=T)
    for a in (X, Y, W):
        a.setflags(write=False)
    return o, trees, flat, X, Y, W


@functools.lru_cache(maxsize=None)
def predictions(T, n=N):
    o, trees, flat, X, Y, W = problem(T, n)
    with np.errstate(all="ignore"):
        yhat, ok = oracle.eval_trees(flat, X, dtype=T)
        osp = output_spread(trees, o, X, T)
    return yhat, ok, osp


@functools.lru_cache(maxsize=None)
def reference(T, loss, weighted, k, lo=0, hi=N):
    """The oracle's (Σ w·ℓ in float64, loss in T, did_succeed, conditioned spread of the mean loss)
    of every tree against target k alone, over rows [lo, hi)."""
    T = np.dtype(T).type
    o, trees, flat, X, Y, W = problem(T)
    Xs, y = X[:, lo:hi], Y[k, lo:hi]
    w = W[k, lo:hi] if weighted else None
    wsum = float(hi - lo) if w is None else float(w.astype(np.float64).sum())
    with np.errstate(all="ignore"):
        if loss.kind >= K.MARGIN_LOSS_BEGIN:  # (all rows only: did_succeed is that of the whole X)
            assert (lo, hi) == (0, N)
            yhat, rok, osp = predictions(T)
            e = M.value(loss.kind, loss.param, yhat * y).astype(np.float64)
            w64 = np.ones(N) if w is None else w.astype(np.float64)
            sums = (e * w64).sum(axis=1)
            spread = (osp * np.abs(y.astype(np.float64)) * w64).sum(axis=1)
            losses = (sums / wsum).astype(T)
        else:
            sums, losses, rok = oracle.eval_loss_batch(flat, Xs, y, w, loss.kind, loss.params, dtype=T)
            spread = loss_spread(trees, o, Xs, y, w, T, loss=loss)
    rok = np.asarray(rok).astype(bool)
    return sums, losses, rok, spread / wsum, wsum


def reference_for(T, loss, weighted, tg, lo=0, hi=N):
    """Per tree, the reference of its own target."""
    per = [reference(T, loss, weighted, k, lo, hi) for k in range(NT)]
    idx = np.arange(len(tg))
    losses = np.stack([p[1] for p in per])[tg, idx]
    rok = np.stack([p[2] for p in per])[tg, idx]
    spread = np.stack([p[3] for p in per])[tg, idx]
    return losses, rok, spread, np.array([p[4] for p in per])


def check_against_oracle(l, ok, ref, rok, spread, T, what, need_failures):
    T = np.dtype(T).type
    assert np.array_equal(ok, rok), (what, np.flatnonzero(ok != rok))
    if need_failures:
        assert 0 < ok.sum() < len(ok), what
    m = ok & np.isfinite(ref)
    with np.errstate(all="ignore"):
        rel = np.abs(l[m].astype(np.float64) - ref[m]) / np.abs(ref[m])
    print(f"{what}: {int(m.sum())} trees compared, max rel {float(np.nanmax(rel)):.3g}")
    assert m.sum() >= (100 if T == np.float32 else 30), (what, int(m.sum()))
    assert_close_conditioned(l[m], ref[m], spread[m], rtol=RTOL[T], msg=what, max_bad_frac=0)
    assert np.all(np.isinf(l[~ok])), what


def target_patterns(ntrees, seed):
    rng = np.random.default_rng(seed)
    return {"random": rng.integers(0, NT, ntrees).astype(np.int32),
            "all-on-2": np.full(ntrees, 2, dtype=np.int32),
            "none-on-1": rng.choice([0, 2], ntrees).astype(np.int32)}


# ---- 1. the fused call against the oracle ----------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("T", DTYPES)
def test_fused_call_matches_the_oracle(gpu_ctx, T, weighted, loss):
    o, trees, flat, X, Y, W = problem(T)
    mds = srhip.MultiDataset(X, Y, weights=W if weighted else None)
    dev = mds.device()
    prog = srhip.Program(dev.ctx, flat, T, interpreted=True)
    for name, tg in target_patterns(len(trees), 143).items():
        what = f"fused {np.dtype(T).name} weighted={weighted} kind={loss.kind} targets={name}"
        sums, wsum, ok = prog.eval_loss_targets(dev, loss.kind, tg, loss.params)
        assert dev.ctx.last_tree_code() == 0 and "wide" not in dev.ctx.last_kernel_name(), what
        ref, rok, spread, rws = reference_for(T, loss, weighted, tg)
        assert wsum == pytest.approx(rws, rel=1e-12), what  # Σ W[k], or the row count
        if not weighted:
            assert np.all(wsum == N)
        with np.errstate(all="ignore"):
            l = (sums / wsum[tg]).astype(T)
        l[~ok] = np.inf
        assert np.all(np.isnan(sums[~ok])), what
        check_against_oracle(l, ok, ref, rok, spread, T, what, T == np.float64)
        # the public function takes the same path below the tree-code bar
        o2 = srhip.Options(binary_operators=list(o.binary_operators), unary_operators=list(o.unary_operators),
                           elementwise_loss=loss)
        l2, ok2 = srhip.eval_loss_batch_ok(trees, mds, o2, targets=tg)
        assert np.array_equal(ok2, ok) and np.array_equal(bits(l2), bits(l)), what


# ---- 2. views are exact -----------------------------------------------------------------------
@pytest.mark.parametrize("T", DTYPES)
def test_views_equal_plain_datasets_bit_for_bit(gpu_ctx, T):
    """Loss, ok, gradients and per-row outputs of mds.target(k) against a Dataset made of
    (X, Y[k], W[k]): the same kernels on the same geometry. 159 trees (interpreted) and a
    300-tree program (tree code)."""
    o, trees, flat, X, Y, W = problem(T)
    otc = srhip.Options(binary_operators=F32_OPS[0], unary_operators=F32_OPS[1])  # operators tree code holds
    big = list(srhip.random_population(300, otc, NFEAT, T, seed=144))
    ctx = gpu_ctx
    progs = [srhip.Program(ctx, flat, T), srhip.Program(ctx, srhip.flatten(big, otc, dtype=T), T)]
    assert progs[0].pass_info()["tree_code"] == 0 and progs[1].pass_info()["tree_code"] > 0

    def run(prog, ds, outputs):
        res = []
        for loss in (L2, HUBER):
            s, ws, ok = prog.eval_loss(ds, loss.kind, loss.params)
            res.append((prog.pass_info(), ctx.last_tree_code(), ctx.last_kernel_name(), bits(s[ok]), ws, ok.copy()))
        s, g, ws, ok = prog.eval_loss_grad(ds, L2.kind, L2.params)
        res.append((prog.pass_info(), ctx.last_kernel_name(), bits(s[ok]), g.tobytes(), ws, ok.copy()))
        s, ws, ok = prog.eval_loss(ds, L2.kind, L2.params, np.arange(0, N, 7))
        res.append((bits(s[ok]), ws, ok.copy()))
        if outputs:
            out, ok = prog.eval_tree_array(ds)
            res.append((ctx.last_kernel_name(), bits(out[ok]), ok.copy()))
        return res

    for weighted in (False, True):
        mds = srhip.MultiDataset(X, Y, weights=W if weighted else None)
        for k in range(NT):
            view = mds.target(k).device()
            plain = srhip.Dataset(X, Y[k], weights=W[k] if weighted else None).device()
            assert view.info() == plain.info()
            assert mds.target(k).avg_y == srhip.Dataset(X, Y[k], weights=W[k] if weighted else None).avg_y
            for prog in progs:
                if not weighted and k == 0:
                    # a program builds its gradient programs and Huber's tree code at first use:
                    # after one round pass_info stands still
                    run(prog, plain, False)
                ra, rb = run(prog, view, prog is progs[0]), run(prog, plain, prog is progs[0])
                for i, (a, b) in enumerate(zip(ra, rb)):
                    for j, (x, y) in enumerate(zip(a, b)):
                        same = np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
                        assert same, (k, weighted, prog.ntrees, i, j, "" if isinstance(x, np.ndarray) else (x, y))
                if prog is progs[1]:
                    assert ra[0][1] > 0  # the 300-tree program ran as tree code on the view
        # a kept view outlives the MultiDataset and its device copy
        view = mds.target(1).device()
        prog = progs[0]
        s0, _, ok0 = prog.eval_loss(view, L2.kind, L2.params)
        s0, ok0 = s0.copy(), ok0.copy()
        del mds
        import gc

        gc.collect()
        s1, _, ok1 = prog.eval_loss(view, L2.kind, L2.params)
        assert np.array_equal(ok0, ok1) and np.array_equal(bits(s0[ok0]), bits(s1[ok1]))


def test_c_level_view_outlives_its_parent(gpu_ctx):
    """srhip_dataset_destroy on the parent first: the view still scores, then frees the memory."""
    T = np.float32
    o, trees, flat, X, Y, W = problem(T)
    parent = srhip.MultiDeviceDataset(gpu_ctx, X, Y, W)
    assert parent.target_info(2)[0] == pytest.approx(float(W[2].astype(np.float64).sum()), rel=1e-12)
    n = C.c_int32()
    _lib.check(_lib.lib().srhip_dataset_targets(parent.handle, C.byref(n)))
    assert n.value == NT
    view = parent.view(2)
    _lib.check(_lib.lib().srhip_dataset_targets(view.handle, C.byref(n)))
    assert n.value == 1
    prog = srhip.Program(gpu_ctx, flat, T)
    s0, w0, ok0 = prog.eval_loss(view, L2.kind)
    s0, ok0 = s0.copy(), ok0.copy()
    _lib.check(_lib.lib().srhip_dataset_destroy(parent.handle))
    parent.handle = None
    s1, w1, ok1 = prog.eval_loss(view, L2.kind)
    assert w0 == w1 and np.array_equal(ok0, ok1) and np.array_equal(bits(s0[ok0]), bits(s1[ok1]))
    ref = reference(T, L2, True, 2)
    assert np.array_equal(ok1, ref[2])


# ---- 3. K = 1 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", [pytest.param(L2, id="L2"), pytest.param(HUBER, id="Huber")])
@pytest.mark.parametrize("T", DTYPES)
def test_one_target_fused_equals_eval_loss_bit_for_bit(gpu_ctx, T, loss):
    """The fused call on a one-target dataset, all targets 0, against srhip_eval_loss of the
    same trees (an interpreted program) on the plain dataset: the same rows in the same order
    through the same routines."""
    o, trees, flat, X, Y, W = problem(T)
    tg = np.zeros(len(trees), dtype=np.int32)
    for weighted in (False, True):
        w = W[:1] if weighted else None
        one = srhip.MultiDeviceDataset(gpu_ctx, X, Y[:1], w)
        plain = srhip.DeviceDataset(gpu_ctx, X, Y[0], None if w is None else w[0])
        prog = srhip.Program(gpu_ctx, flat, T, interpreted=True)
        s1, w1, ok1 = prog.eval_loss_targets(one, loss.kind, tg, loss.params)
        s1, ok1 = s1.copy(), ok1.copy()
        s0, w0, ok0 = prog.eval_loss(plain, loss.kind, loss.params)
        assert w1.shape == (1,) and w1[0] == w0
        assert np.array_equal(ok0, ok1)
        assert np.array_equal(bits(s0[ok0]), bits(s1[ok1])), (weighted, np.flatnonzero(s0[ok0] != s1[ok1]))
        # and a one-target dataset is an ordinary dataset for the single-target calls
        s2, w2, ok2 = prog.eval_loss(one, loss.kind, loss.params)
        assert w2 == w0 and np.array_equal(ok2, ok0) and np.array_equal(bits(s2[ok2]), bits(s0[ok0]))


# ---- 4. the LDS boundary ------------------------------------------------------------------------
def boundary_case(ctx, T, nfeat, ntg, rtol):
    o, trees, flat, X, y, w = WC.problem(T, nfeat, 700, 200)
    rng = np.random.default_rng(145)
    Y = np.stack([y] + [(y * T(0.5 + k) + X[k]).astype(T) for k in range(1, ntg)])
    Wt = np.stack([w] + [np.abs(rng.standard_normal(700)).astype(T) + T(0.01) for _ in range(1, ntg)])
    mds = srhip.MultiDataset(X, Y, weights=Wt)
    tg = rng.integers(0, ntg, len(trees)).astype(np.int32)
    l, ok = srhip.eval_loss_batch_ok(trees, mds, o, targets=tg, fused=True)
    fused_name = ctx.last_kernel_name()
    refs, roks, sps = [], [], []
    view_names = []
    lv = np.zeros(len(trees), dtype=T)
    okv = np.zeros(len(trees), dtype=bool)
    for k in range(ntg):
        with np.errstate(all="ignore"):
            _, r, rk = oracle.eval_loss_batch(flat, X, Y[k], Wt[k], L2.kind, L2.params, dtype=T)
            sp = loss_spread(trees, o, X, Y[k], Wt[k], T) / float(Wt[k].astype(np.float64).sum())
        refs.append(r), roks.append(rk.astype(bool)), sps.append(sp)
        a, b = srhip.eval_loss_batch_ok(trees, mds.target(k), o)
        view_names.append(ctx.last_kernel_name())
        lv[tg == k], okv[tg == k] = a[tg == k], b[tg == k]
    idx = np.arange(len(tg))
    ref, rok, spread = np.stack(refs)[tg, idx], np.stack(roks)[tg, idx], np.stack(sps)[tg, idx]
    for got, gok, what in ((l, ok, "fused"), (lv, okv, "views")):
        assert np.array_equal(gok, rok), what
        m = gok & np.isfinite(ref)
        assert m.sum() >= 150, (what, int(m.sum()))
        assert_close_conditioned(got[m], ref[m], spread[m], rtol=rtol, msg=f"{what} nfeat={nfeat}", max_bad_frac=0)
    return fused_name, view_names


def test_lds_boundary_f32_75_features_4_weighted_targets(gpu_ctx):
    """75 features + 4·2 columns = 83 arrays: past the 79 a Float32 shallow tile holds, so the
    fused call runs wide; a view's 77 arrays fit and it runs the LDS kernels."""
    fused, views = boundary_case(gpu_ctx, np.float32, 75, 4, 1e-5)
    assert "wide" in fused, fused
    assert all("wide" not in v for v in views), views


def test_wide_fused_f64_100_features(gpu_ctx):
    fused, _ = boundary_case(gpu_ctx, np.float64, 100, 3, 1e-9)
    assert "wide" in fused, fused


# ---- 5. row sets with targets -------------------------------------------------------------------
@pytest.mark.parametrize("bs", [50, 700])
@pytest.mark.parametrize("T", DTYPES)
def test_rowsets_with_targets_match_the_oracle_tree_by_tree(gpu_ctx, T, bs):
    o, trees, flat, X, Y, W = problem(T)
    rng = np.random.default_rng(146)
    tg = rng.integers(0, NT, len(trees)).astype(np.int32)
    rows = [rng.integers(0, N, bs) for _ in trees]
    rows[0][:] = rows[0][0]  # one sample that is a single row repeated
    rows[1][: bs // 2] = rows[1][bs // 2:bs // 2 * 2]  # halves repeated
    for weighted in (False, True):
        mds = srhip.MultiDataset(X, Y, weights=W if weighted else None)
        l, ok = srhip.eval_loss_batch_rowsets(trees, mds, o, rows, targets=tg)
        dev = mds.device()
        prog = srhip.Program(dev.ctx, flat, T, interpreted=True)
        _, ws, _ = prog.eval_loss_rowsets_targets(dev, L2.kind, tg, np.stack(rows))
        ref = np.zeros(len(trees), dtype=T)
        rok = np.zeros(len(trees), dtype=bool)
        sp = np.zeros(len(trees))
        rws = np.zeros(len(trees))
        with np.errstate(all="ignore"):
            for t, (tree, r) in enumerate(zip(trees, rows)):
                y = Y[tg[t]]
                w = W[tg[t]] if weighted else None
                _, lt, kt = oracle.eval_loss_batch(flat.take([t]), X, y, w, L2.kind, L2.params, row_idx=r, dtype=T)
                ref[t], rok[t] = lt[0], kt[0]
                rws[t] = bs if w is None else w[r].astype(np.float64).sum()
                sp[t] = loss_spread([tree], o, X[:, r], y[r], None if w is None else w[r], T)[0] / rws[t]
        assert np.allclose(ws, rws, rtol=1e-12)
        check_against_oracle(l, ok, ref, rok, sp, T, f"rowsets {np.dtype(T).name} bs={bs} weighted={weighted}",
                             T == np.float64)


# ---- 6. errors ------------------------------------------------------------------------------------
def test_errors(gpu_ctx):
    T = np.float32
    o, trees, flat, X, Y, W = problem(T)
    dev = srhip.MultiDeviceDataset(gpu_ctx, X, Y, W)
    prog = srhip.Program(gpu_ctx, flat, T, interpreted=True)
    nt = len(trees)
    par = np.zeros(1)
    for bad in (NT, -1):
        tg = np.zeros(nt, dtype=np.int32)
        tg[nt // 2] = bad
        sums = np.full(nt, 123.0)
        wsum = np.full(NT, 456.0)
        ok = np.full(nt, 7, dtype=np.uint8)
        rc = _lib.lib().srhip_eval_loss_targets(dev.handle, prog.handle, L2.kind, par.ctypes.data, tg.ctypes.data,
                                                sums.ctypes.data, wsum.ctypes.data, ok.ctypes.data)
        assert rc == _lib.ERR_INVALID
        assert np.all(sums == 123.0) and np.all(wsum == 456.0) and np.all(ok == 7)
        idx = np.zeros((nt, 4), dtype=np.int64)
        wt = np.full(nt, 456.0)
        rc = _lib.lib().srhip_eval_loss_rowsets_targets(dev.handle, prog.handle, L2.kind, par.ctypes.data,
                                                        tg.ctypes.data, idx.ctypes.data, 4, sums.ctypes.data,
                                                        wt.ctypes.data, ok.ctypes.data)
        assert rc == _lib.ERR_INVALID
        assert np.all(sums == 123.0) and np.all(wt == 456.0) and np.all(ok == 7)
    # a multi-target dataset in a single-target entry point: INVALID, and the message says what to do
    with pytest.raises(srhip.SrhipError) as e:
        prog.eval_loss(dev, L2.kind)
    assert e.value.code == _lib.ERR_INVALID and "view" in str(e.value)
    with pytest.raises(srhip.SrhipError) as e:
        prog.eval_loss_grad(dev, L2.kind)
    assert e.value.code == _lib.ERR_INVALID
    # an expression loss: UNSUPPORTED from the fused calls, a correct result from a view
    xl = EL.expr_loss("SQ")
    tg = np.zeros(nt, dtype=np.int32)
    with pytest.raises(srhip.Unsupported):
        prog.eval_loss_targets(dev, xl.kind, tg)
    with pytest.raises(srhip.Unsupported):
        prog.eval_loss_rowsets_targets(dev, xl.kind, tg, np.zeros((nt, 4), dtype=np.int64))
    s, ws, ok = prog.eval_loss(dev.view(1), xl.kind)
    s, ok = s.copy(), ok.copy()
    s0, ws0, ok0 = prog.eval_loss(srhip.DeviceDataset(gpu_ctx, X, Y[1], W[1]), xl.kind)
    assert ws == ws0 and np.array_equal(ok, ok0) and np.array_equal(bits(s[ok]), bits(s0[ok0]))
    assert np.array_equal(ok, reference(T, L2, False, 1)[2])
    # the Python surface
    mds = srhip.MultiDataset(X, Y, weights=W)
    with pytest.raises(ValueError):
        srhip.eval_loss_batch_ok(trees, mds, o)
    with pytest.raises(ValueError):
        srhip.eval_loss_batch_rowsets(trees, mds, o, [np.arange(4)] * nt)
    with pytest.raises(ValueError):
        srhip.eval_loss_batch_ok(trees, mds, o, targets=np.full(nt, NT))


# ---- 7. a row shard -----------------------------------------------------------------------------
@pytest.mark.parametrize("T", DTYPES)
def test_row_shard(gpu_ctx, T):
    o, trees, flat, X, Y, W = problem(T)
    lo, hi = 1000, N
    dev = srhip.MultiDeviceDataset(gpu_ctx, X, Y, W, lo, hi)
    assert dev.info()["rows"] == hi - lo
    prog = srhip.Program(gpu_ctx, flat, T, interpreted=True)
    tg = np.random.default_rng(147).integers(0, NT, len(trees)).astype(np.int32)
    sums, wsum, ok = prog.eval_loss_targets(dev, L2.kind, tg, L2.params)
    ref, rok, spread, rws = reference_for(T, L2, True, tg, lo, hi)
    assert wsum == pytest.approx(rws, rel=1e-12)
    with np.errstate(all="ignore"):
        l = (sums / wsum[tg]).astype(T)
    l[~ok] = np.inf
    check_against_oracle(l, ok, ref, rok, spread, T, f"row shard {np.dtype(T).name}", T == np.float64)


# ---- the two paths of the public function ---------------------------------------------------------
def test_views_and_fused_paths_of_the_public_function(gpu_ctx):
    """900 trees, 300 per target: fused=False regroups by target and scores each group on its
    view (tree code), the default (up to FUSED_TARGETS_MAX_TREES trees) is the fused call."""
    T = np.float32
    o, trees, flat, X, Y, W = problem(T)
    big = list(srhip.random_population(3 * 300, o, NFEAT, T, seed=148))
    tg = np.random.default_rng(149).permutation(np.repeat(np.arange(NT), 300)).astype(np.int32)
    mds = srhip.MultiDataset(X, Y, weights=W)
    assert len(big) <= srhip.interface.FUSED_TARGETS_MAX_TREES
    l, ok = srhip.eval_loss_batch_ok(big, mds, o, targets=tg, fused=False)
    assert mds.device().ctx.last_tree_code() > 0  # 300 trees per target: tree code on the views
    lf, okf = srhip.eval_loss_batch_ok(big, mds, o, targets=tg)
    assert mds.device().ctx.last_tree_code() == 0
    lf2, okf2 = srhip.eval_loss_batch_ok(big, mds, o, targets=tg, fused=True)
    assert np.array_equal(okf, okf2) and np.array_equal(bits(lf), bits(lf2))
    assert np.array_equal(ok, okf)
    fin = ok & np.isfinite(l) & np.isfinite(lf)
    bigflat = srhip.flatten(big, o, dtype=T)
    for k in range(NT):
        m = fin & (tg == k)
        sub = [t for t, q in zip(big, m) if q]
        sp = loss_spread(sub, o, X, Y[k], W[k], T) / float(W[k].astype(np.float64).sum())
        with np.errstate(all="ignore"):
            _, ref, rok = oracle.eval_loss_batch(bigflat.take(np.flatnonzero(m)), X, Y[k], W[k], L2.kind, L2.params,
                                                 dtype=T)
        for got in (l[m], lf[m]):
            assert_close_conditioned(got, ref, sp, rtol=1e-5, msg=f"views / fused, target {k}", max_bad_frac=0)
