"""Constant gradients and constant optimisation on per-tree row samples:
srhip_eval_loss_grad_rowsets and srhip_optimize_constants_rowsets.

The gradient kernel's segment mode runs one (tree, tangent group) per workgroup
over the tree's gathered sample with the tiles, lane sums, shuffle tree and
row-group sum of a dataset made of that sample. So the main check takes no
tolerance: tree t of a row-set call equals entry t of the same program's
srhip_eval_loss_grad on srhip.Dataset(X[:, idx_t], y[idx_t], w[idx_t]) bit for
bit (a program below 256 trees: no gradient tree code on either side). The
optimiser's per-candidate algebra is independent per tree, so optimising tree
t on its sample equals optimising it alone on that dataset, bit for bit too.
An independent check against the oracle's forward-mode gradients follows.

Batch sizes: 50 (one tile, 462 padding rows of a 512-row segment), 700 (several
tiles, the last partial), 9000 (a 16384-row segment, more than one row group).
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import srhip
from expr_loss_cases import e4, loss_options
from numerics import assert_close_conditioned, loss_spread
from srhip import Node
from srhip import constants as K
from test_constant_optimization import problem

pytestmark = pytest.mark.gpu

N = 3000
OPS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
# with an operator that fails on some rows of X ~ U(-3, 3): did_succeed depends on the sample
NAN_OPS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "safe_sqrt"])
# oracle population (test 2): chosen on the CPU with the oracle so that, on these
# samples, at least 30 trees succeed and at least 5 fail at both batch sizes
ORACLE_SEED = 45


def deep_tree(depth, rng):
    """As tests/test_rowsets_gpu.py builds them: more than 4 stack slots."""
    if depth == 0:
        return Node(feature=int(rng.integers(1, 4))) if rng.random() < 0.7 else Node(val=float(rng.standard_normal()))
    return Node(int(rng.integers(1, 4)), deep_tree(depth - 1, rng), deep_tree(depth - 1, rng))


def chain(o, nconst):
    """c1·cos(x4) + c2·x1·x1 + c3·x2 + …: nconst constants, at most 4 stack slots."""
    B, U = o.make_binary, o.make_unary
    terms = [lambda: U("cos", Node("x4")), lambda: B("*", Node("x1"), Node("x1")), lambda: Node("x2"),
             lambda: Node("x3"), lambda: Node("x5")]
    t = B("*", Node(val=1.0), terms[0]())
    for k in range(1, nconst):
        t = B("+", t, B("*", Node(val=0.5 + 0.25 * k), terms[k % len(terms)]()))
    return t


def hand_trees(o):
    rng = np.random.default_rng(5)
    B = o.make_binary
    trees = [chain(o, k) for k in (1, 2, 4, 5, 9)]  # one, two and three items; every tangent width
    deep = []
    while len(deep) < 2:
        t = deep_tree(6, rng)
        if len(srhip.get_constants(t)) > 0:
            deep.append(t)
    trees += deep
    trees.append(B("*", Node("x1"), Node("x1")))  # no constants
    trees.append(B("+", Node("x2"), Node(val=np.inf)))  # static failure
    return trees


def data(T, hinge=False):
    rng = np.random.default_rng(101)
    X = rng.standard_normal((5, N)).astype(T) if T == np.float32 else rng.uniform(-3, 3, (5, N))
    y = (2 * np.cos(X[3]) + X[0] * X[0] - 2).astype(T)
    if hinge:
        y = np.where(y > 0, 1, -1).astype(T)
    w = np.abs(rng.standard_normal(N)).astype(T)
    return X, y, w


def samples(ntrees, bs, seed=102):
    rng = np.random.default_rng(seed + bs)
    rows = rng.integers(0, N, (ntrees, bs))  # with replacement
    rows[0, :] = rows[0, 0]  # one row repeated
    rows[1, : bs // 2] = rows[1, bs // 2: bs // 2 * 2]  # halves repeated
    return rows


def population(T):
    o = srhip.Options(**OPS)
    return o, srhip.random_population(40, o, 5, T, seed=42) + hand_trees(o)


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8) if a.dtype != bool else a,
                                                 b.view(np.uint8) if b.dtype != bool else b)


def check_bit_for_bit(T, bs, wide_env):
    """Tree t of the row-set call == entry t of eval_loss_grad on tree t's sample as a dataset."""
    o, trees = population(T)
    flat = srhip.flatten(trees, o, dtype=T)
    co = flat.const_off
    assert len(trees) < 256 and {int(co[t + 1] - co[t]) for t in range(len(trees))} >= {0, 1, 2, 4, 5, 9}
    rows = samples(len(trees), bs)
    lo = loss_options()
    cells = [(False, [srhip.L2DistLoss(), srhip.HuberLoss(1.0), srhip.ExprLoss(e4(lo), lo)]),
             (True, [srhip.L1HingeLoss()])]
    ctx = srhip.get_context(0)
    for weighted in (False, True):
        for hinge, losses in cells:
            X, y, w = data(T, hinge)
            wt = w if weighted else None
            ds = srhip.Dataset(X, y, weights=wt)
            dev = ds.device()
            prog = srhip.engine.Program(dev.ctx, flat, T)
            per_tree = [srhip.Dataset(X[:, r], y[r], weights=None if wt is None else wt[r]).device() for r in rows]
            for loss in losses:
                what = f"{T.__name__} bs={bs} weighted={weighted} loss={type(loss).__name__} wide={wide_env}"
                s, g, ws, ok = prog.eval_loss_grad_rowsets(dev, loss.kind, rows, loss.params)
                name = ctx.last_kernel_name()
                assert "_seg<" in name and ("wide" in name) == wide_env, (what, name)
                assert ctx.last_tree_code() == 0
                for t in range(len(trees)):
                    s1, g1, w1, ok1 = prog.eval_loss_grad(per_tree[t], loss.kind, loss.params)
                    assert ok[t] == ok1[t], (what, t)
                    assert np.array_equal(s[t:t + 1], s1[t:t + 1], equal_nan=True), (what, t, s[t], s1[t])
                    assert bits_equal(g[co[t]:co[t + 1]], g1[co[t]:co[t + 1]]), (what, t)
                    assert ws[t] == w1, (what, t)
                    if not ok[t]:
                        assert np.isnan(s[t]) and np.all(np.isnan(g[co[t]:co[t + 1]]))
                assert ok[:-1].sum() >= 30 and not ok[-1], what  # the Inf constant fails statically


@pytest.mark.parametrize("bs", [50, 700, 9000])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_rowset_gradients_equal_per_sample_datasets_bit_for_bit(gpu_ctx, T, bs):
    check_bit_for_bit(T, bs, False)


@pytest.mark.parametrize("bs", [50, 700])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_rowset_gradients_wide_bit_for_bit(gpu_ctx, monkeypatch, T, bs):
    monkeypatch.setenv("SRHIP_WIDE", "1")  # read per call: both sides run the wide variants
    check_bit_for_bit(T, bs, True)


@pytest.mark.parametrize("bs", [50, 700])
def test_rowset_gradients_match_oracle(gpu_ctx, bs):
    """Float64, L2: Σ 2 r_i g_i and the loss against the oracle's eval_grad_consts on X[:, idx_t].
    Gradient bar: 2e-10 · Σ_i 2(|ŷ_i| + |y_i|)|g_i|, from the per-row 1e-10 bar the engine's ŷ and
    ∂ŷ/∂c are held to (tests/test_gradients.py) plus the fp64 sum."""
    T = np.float64
    o = srhip.Options(**NAN_OPS)
    trees = srhip.random_population(40, o, 5, T, seed=ORACLE_SEED) + hand_trees(o)
    X, y, _ = data(T)
    rows = samples(len(trees), bs)
    flat = srhip.flatten(trees, o, dtype=T)
    co = flat.const_off
    ds = srhip.Dataset(X, y)
    dev = ds.device()
    prog = srhip.engine.Program(dev.ctx, flat, T)
    s, g, ws, ok = prog.eval_loss_grad_rowsets(dev, K.LOSS["L2"], rows)
    assert np.all(ws == bs)
    nok = nfail = 0
    for t in range(len(trees)):
        k, a, c = flat.tree(t)
        r = rows[t]
        out, gr, rok = oracle.eval_grad_consts(k, a, np.asarray(c, dtype=T), X[:, r], len(c))
        assert bool(rok) == bool(ok[t]), f"did_succeed of tree {t} differs from the oracle"
        if not rok:
            nfail += 1
            continue
        nok += 1
        res = out - y[r]
        sp = loss_spread([trees[t]], o, X[:, r], y[r], None, T)[0]
        if not np.isfinite(np.sum(res * res)):
            assert not np.isfinite(s[t]), t
            continue
        assert_close_conditioned(s[t:t + 1], np.array([np.sum(res * res)]), np.array([sp]), rtol=1e-9,
                                 msg=f"loss sum of tree {t}")
        if len(c):
            gref = 2.0 * (gr @ res)
            bar = 2e-10 * np.sum(2.0 * (np.abs(out) + np.abs(y[r])) * np.abs(gr), axis=1)
            gt = g[co[t]:co[t + 1]]
            fin = np.isfinite(bar) & np.isfinite(gref)  # (a sum that overflows fp64 has no bar: not finite here either)
            err = np.abs(gt[fin] - gref[fin])
            assert np.all(err <= bar[fin]), (t, err, bar)
            assert not np.isfinite(gt[~fin]).any(), (t, gt, gref)
    assert nok >= 30 and nfail >= 5, (nok, nfail)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_did_succeed_is_per_sample(gpu_ctx, T):
    o = srhip.Options(**NAN_OPS)
    tree = lambda: o.make_unary("safe_sqrt", o.make_binary("*", Node(val=1.0), Node("x1")))
    trees = [tree(), tree()]
    X, y, w = data(T)
    pos, neg = np.flatnonzero(X[0] > 0), np.flatnonzero(X[0] < 0)
    rng = np.random.default_rng(3)
    bs = 50
    rows = np.stack([rng.choice(pos, bs), rng.choice(pos, bs)])
    rows[1, 17] = neg[0]
    ds = srhip.Dataset(X, y, weights=w)
    dev = ds.device()
    flat = srhip.flatten(trees, o, dtype=T)
    prog = srhip.engine.Program(dev.ctx, flat, T)
    s, g, ws, ok = prog.eval_loss_grad_rowsets(dev, K.LOSS["L2"], rows)
    assert list(ok) == [True, False]
    assert np.isnan(s[1]) and np.isnan(g[1]) and np.isfinite(s[0]) and np.isfinite(g[0])
    d0 = srhip.Dataset(X[:, rows[0]], y[rows[0]], weights=w[rows[0]]).device()
    s1, g1, w1, ok1 = prog.eval_loss_grad(d0, K.LOSS["L2"])
    assert ok1[0] and s[0] == s1[0] and g[0] == g1[0] and ws[0] == w1
    # a sample that is one row repeated, and one with halves repeated
    rows2 = np.stack([np.full(bs, pos[5]), np.concatenate([rows[0, :25], rows[0, :25]])])
    s2, g2, ws2, ok2 = prog.eval_loss_grad_rowsets(dev, K.LOSS["L2"], rows2)
    assert ok2.all()
    for t in range(2):
        dt = srhip.Dataset(X[:, rows2[t]], y[rows2[t]], weights=w[rows2[t]]).device()
        s3, g3, w3, ok3 = prog.eval_loss_grad(dt, K.LOSS["L2"])
        assert s2[t] == s3[t] and g2[t] == g3[t] and ws2[t] == w3


def opt_trees(T):
    o, _, _, trees = problem(T)
    pop = [t for t in srhip.random_population(60, o, 5, T, seed=11, maxsize=15) if len(srhip.get_constants(t)) > 0]
    return o, trees + pop[:20]


@pytest.mark.parametrize("bs", [50, 700])
@pytest.mark.parametrize("algorithm", ["BFGS", "NelderMead"])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_rowset_optimiser_equals_per_sample_optimiser_bit_for_bit(gpu_ctx, T, algorithm, bs):
    """Tree t optimised on its sample == tree t optimised alone on a dataset of that sample, with
    its slice of the same start noise: constants, losses, converged, num_evals."""
    o, trees = opt_trees(T)
    o.optimizer_algorithm = algorithm
    X, y, w = data(T)
    wt = w if algorithm == "BFGS" else None  # both weight paths
    rows = samples(len(trees), bs, seed=202)
    flat = srhip.flatten(trees, o, dtype=T)
    nre = o.optimizer_nrestarts
    noise = srhip.constant_optimization.start_noise(flat, nre, np.random.default_rng(9))
    noff = np.concatenate([[0], np.cumsum(nre * np.diff(flat.const_off))])
    ds = srhip.Dataset(X, y, weights=wt)
    mine = [t.copy() for t in trees]
    res = srhip.optimize_constants_batch(ds, mine, o, noise=noise, row_idx=rows)
    prof = srhip.constant_optimization.last_profile()
    assert prof["n_segment_evals"] == prof["n_loss"] + prof["n_grad"] > 0
    assert gpu_ctx.last_tree_code() == 0
    assert res.converged.any()
    for t, tree in enumerate(trees):
        r = rows[t]
        alone = [tree.copy()]
        dt = srhip.Dataset(X[:, r], y[r], weights=None if wt is None else wt[r])
        ref = srhip.optimize_constants_batch(dt, alone, o, noise=noise[noff[t]:noff[t + 1]])
        what = f"{T.__name__} {algorithm} bs={bs} tree {t}"
        assert bits_equal(np.asarray(srhip.get_constants(mine[t]), dtype=T),
                          np.asarray(srhip.get_constants(alone[0]), dtype=T)), what
        assert np.array_equal(res.losses[t:t + 1], ref.losses, equal_nan=True), (what, res.losses[t], ref.losses)
        assert res.converged[t] == ref.converged[0], what
        assert res.num_evals[t] == ref.num_evals[0], what


@pytest.mark.parametrize("T", [np.float64, np.float32])
def test_rowset_optimiser_recovers_constants(gpu_ctx, T):
    """problem() at 100 000 noise-free rows, samples of 1000: the 3-constant tree converges to
    [2, 1, -2] at test_engine_optimizer_matches_oracle_driver's atol, on segment kernels only."""
    o, X, y, trees = problem(T, n=100_000)
    rows = np.random.default_rng(4).integers(0, X.shape[1], (len(trees), 1000))
    ds = srhip.Dataset(X, y)
    res = srhip.optimize_constants_batch(ds, trees, o, rng=np.random.default_rng(0), row_idx=rows)
    atol = 1e-6 if T == np.float64 else 2e-3
    assert res.converged[0]
    assert np.allclose(srhip.get_constants(trees[0]), [2.0, 1.0, -2.0], atol=atol)
    assert res.losses[0] < (1e-10 if T == np.float64 else 1e-5)
    prof = srhip.constant_optimization.last_profile()
    assert prof["n_grad"] > 0 and prof["n_segment_evals"] == prof["n_loss"] + prof["n_grad"]
    assert gpu_ctx.last_tree_code() == 0
    # the gradient launches report the segment kernel (the loss-only ones the row-set eval kernel)
    dev = ds.device()
    prog = srhip.engine.Program(dev.ctx, srhip.flatten(trees, o, dtype=T), T, interpreted=True)
    prog.eval_loss_grad_rowsets(dev, K.LOSS["L2"], rows)
    tn = "float" if T == np.float32 else "double"
    assert gpu_ctx.last_kernel_name() == f"grad_kernel_seg<{tn}>" and gpu_ctx.last_tree_code() == 0


def test_rules(gpu_ctx):
    T = np.float32
    o, X, y, trees = problem(T)
    n = X.shape[1]
    ds = srhip.Dataset(X, y)
    dev = ds.device()
    flat = srhip.flatten(trees, o, dtype=T)
    prog = srhip.engine.Program(dev.ctx, flat, T)
    good = np.zeros((3, 4), dtype=np.int64)
    bad = good.copy()
    bad[2, 3] = n  # an index equal to rows
    with pytest.raises(srhip.SrhipError) as e:
        prog.eval_loss_grad_rowsets(dev, K.LOSS["L2"], bad)
    assert e.value.code == srhip._lib.ERR_INVALID
    with pytest.raises(srhip.SrhipError) as e:
        srhip.optimize_constants_batch(ds, [t.copy() for t in trees], o, rng=np.random.default_rng(0), row_idx=bad)
    assert e.value.code == srhip._lib.ERR_INVALID
    with pytest.raises(ValueError):  # a short row_idx: the shape check eval_loss_rowsets has
        prog.eval_loss_grad_rowsets(dev, K.LOSS["L2"], good[:2])
    # a null row_idx, and a negative batch size, at the C entry
    nc = int(flat.const_off[-1])
    s, g, ws, ok = np.zeros(3), np.zeros(nc), np.zeros(3), np.zeros(3, dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = srhip._lib.lib()
    assert lib.srhip_eval_loss_grad_rowsets(dev.handle, prog.handle, 0, None, None, 4, p(s), p(g), p(ws),
                                            p(ok)) == srhip._lib.ERR_INVALID
    assert lib.srhip_eval_loss_grad_rowsets(dev.handle, prog.handle, 0, None, p(good), -1, p(s), p(g), p(ws),
                                            p(ok)) == srhip._lib.ERR_INVALID
    # batch_size = 0 for the optimiser
    with pytest.raises(srhip.SrhipError) as e:
        srhip.optimize_constants_batch(ds, [t.copy() for t in trees], o, rng=np.random.default_rng(0),
                                       row_idx=np.zeros((3, 0), dtype=np.int64))
    assert e.value.code == srhip._lib.ERR_INVALID
    # a MultiDataset parent
    mds = srhip.MultiDataset(X, np.stack([y, y]))
    with pytest.raises(srhip.SrhipError) as e:
        prog.eval_loss_grad_rowsets(mds.device(), K.LOSS["L2"], good)
    assert e.value.code == srhip._lib.ERR_INVALID
    # batch_size 0 for the gradient call: every sum 0, every tree ok (as no rows)
    s0, g0, w0, ok0 = prog.eval_loss_grad_rowsets(dev, K.LOSS["L2"], np.zeros((3, 0), dtype=np.int64))
    assert ok0.all() and np.all(s0 == 0) and np.all(g0 == 0) and np.all(w0 == 0)
    # an empty tree list
    l, gl, okl = srhip.eval_loss_grad_batch([], ds, o, row_idx=np.zeros((0, 4), dtype=np.int64))
    assert l.shape == (0,) and gl == [] and okl.shape == (0,)
    r = srhip.optimize_constants_batch(ds, [], o, rng=np.random.default_rng(0), row_idx=np.zeros((0, 4), dtype=np.int64))
    assert r.losses.shape == (0,) and r.converged.shape == (0,) and r.num_evals.shape == (0,)
    # the interface divides per tree
    rows = np.random.default_rng(1).integers(0, n, (3, 50))
    l, gl, okl = srhip.eval_loss_grad_batch(trees, ds, o, row_idx=rows)
    s, g, ws, ok = prog.eval_loss_grad_rowsets(dev, K.LOSS["L2"], rows)
    assert np.array_equal(l, (s / ws).astype(T)) and np.array_equal(okl, ok)
    assert all(np.array_equal(gl[t], g[flat.const_off[t]:flat.const_off[t + 1]] / ws[t]) for t in range(3))


def test_tree_code_program_scores_gradient_rowsets_interpreted(gpu_ctx):
    """A 300-tree program: gradient row sets run interpreted and build no gradient tree code; the
    same program's full-data gradient then builds and reports tree code, and row sets stay interpreted."""
    T = np.float32
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    trees = srhip.random_population(300, o, 5, T, seed=71)
    X, y, _ = data(T)
    ds = srhip.Dataset(X, y)
    dev = ds.device()
    prog = srhip.engine.Program(dev.ctx, srhip.flatten(trees, o, dtype=T), T)
    rows = np.random.default_rng(72).integers(0, N, (len(trees), 64))
    s, g, ws, ok = prog.eval_loss_grad_rowsets(dev, K.LOSS["L2"], rows)
    assert gpu_ctx.last_tree_code() == 0 and gpu_ctx.last_kernel_name() == "grad_kernel_seg<float>"
    assert prog.grad_jit_info()["ntrees"] == 0  # none was built for the row-set call
    prog.eval_loss_grad(dev, K.LOSS["L2"])
    assert gpu_ctx.last_tree_code() > 0 and prog.grad_jit_info()["ntrees"] > 0
    s2, g2, ws2, ok2 = prog.eval_loss_grad_rowsets(dev, K.LOSS["L2"], rows)
    assert gpu_ctx.last_tree_code() == 0
    assert np.array_equal(ok, ok2) and np.array_equal(s, s2, equal_nan=True) and np.array_equal(g, g2, equal_nan=True)


def test_group_dataset_with_row_idx_raises():
    gds = object.__new__(srhip.GroupDataset)
    o, X, y, trees = problem(np.float32)
    rows = np.zeros((3, 4), dtype=np.int64)
    with pytest.raises(ValueError):
        srhip.eval_loss_grad_batch(trees, gds, o, row_idx=rows)
    with pytest.raises(ValueError):
        srhip.optimize_constants_batch(gds, trees, o, row_idx=rows)
