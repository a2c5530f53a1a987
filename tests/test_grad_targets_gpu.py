"""Constant gradients and constant optimisation with a target per tree:
srhip_eval_loss_grad_targets, srhip_eval_loss_grad_rowsets_targets and
srhip_optimize_constants_targets on a multi-target dataset.

Over all rows the fused gradient call runs kernel variants of its own whose row
tile holds every column of Y (and W). With one column an item's arithmetic is the
plain kernel's, so K = 1 is compared bit for bit; with K = 3 the tile holds more
arrays, a workgroup covers fewer tiles, and the lane sums group the same per-row
terms differently, so the comparison with the views takes the bar derived below
and an independent check against the oracle follows. Row-set calls gather each
tree's own column and run the row-set kernels: bit for bit against the views.

Shared data: N = 3000 rows (three row groups at R = 1, the last tile partial), 5
features, K = 3 targets, tree t against target t % 3 unless stated.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import constopt_reference as REF
import oracle
import srhip
import wide_cases as WC
from expr_loss_cases import e4, loss_options
from numerics import assert_close_conditioned, loss_spread
from srhip import Node
from srhip import constants as K
from test_grad_rowsets_gpu import N, NAN_OPS, OPS, bits_equal, data, hand_trees, opt_trees, samples

pytestmark = pytest.mark.gpu

NT = 3
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
L2, HUBER, HINGE = srhip.L2DistLoss(), srhip.HuberLoss(1.0), srhip.L1HingeLoss()
EPS = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}


@functools.lru_cache(maxsize=None)
def multi_data(T):
    """(X, Y [3][N], W [3][N]): computed once per dtype, shared, never written to."""
    T = np.dtype(T).type
    X, _, _ = data(T)
    Y = np.stack([2 * np.cos(X[3]) + X[0] * X[0] - 2, X[1] * X[2] + 0.5, np.exp(0.3 * X[4]) - X[0]]).astype(T)
    W = np.abs(np.random.default_rng(103).standard_normal((NT, N))).astype(T)
    for a in (X, Y, W):
        a.setflags(write=False)
    return X, Y, W


def tname(T):
    return "float" if np.dtype(T) == np.float32 else "double"


def cyc(n):
    return (np.arange(n) % NT).astype(np.int32)


# ---- 1. K = 1 is the existing kernel ----------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["lds", "wide"])
@pytest.mark.parametrize("T", DTYPES)
def test_one_target_equals_eval_loss_grad_bit_for_bit(gpu_ctx, monkeypatch, T, wide):
    if wide:
        monkeypatch.setenv("SRHIP_WIDE", "1")  # read per call: both sides run the wide variants
    o = srhip.Options(**OPS)
    trees = srhip.random_population(40, o, 5, T, seed=42) + hand_trees(o)
    flat = srhip.flatten(trees, o, dtype=T)
    tg = np.zeros(len(trees), dtype=np.int32)
    want = f"grad_kernel{'_wide' if wide else ''}_targets<{tname(T)}>"
    for weighted in (False, True):
        for hinge, losses in ((False, [L2, HUBER]), (True, [HINGE])):
            X, y, w = data(T, hinge)
            wt = w if weighted else None
            one = srhip.MultiDeviceDataset(gpu_ctx, X, y[None, :], None if wt is None else wt[None, :])
            plain = srhip.DeviceDataset(gpu_ctx, X, y, wt)
            prog = srhip.Program(gpu_ctx, flat, T, interpreted=True)
            for loss in losses:
                what = f"{tname(T)} weighted={weighted} {type(loss).__name__} wide={wide}"
                s1, g1, w1, ok1 = prog.eval_loss_grad_targets(one, loss.kind, tg, loss.params)
                assert gpu_ctx.last_kernel_name() == want, (what, gpu_ctx.last_kernel_name())
                assert gpu_ctx.last_tree_code() == 0, what
                s0, g0, w0, ok0 = prog.eval_loss_grad(plain, loss.kind, loss.params)
                assert w1.shape == (1,) and w1[0] == w0, what
                assert np.array_equal(ok0, ok1) and ok0[:-1].sum() >= 30 and not ok0[-1], what
                assert bits_equal(s0, s1), (what, np.flatnonzero(s0 != s1))
                assert bits_equal(g0, g1), (what, np.flatnonzero(g0 != g1))
                assert np.all(np.isnan(s1[~ok1])), what


# ---- the Float64 oracle's per-row terms ---------------------------------------------------------
def oracle_terms(flat, t, X, y, w):
    """(ok, ŷ, ∂ŷ/∂c [nc][n], residual) of tree t in Float64 on all rows."""
    k, a, c = flat.tree(t)
    with np.errstate(all="ignore"):
        out, gr, rok = oracle.eval_grad_consts(k, a, np.asarray(c, dtype=np.float64), np.asarray(X, dtype=np.float64),
                                               len(c))
    return bool(rok), out, gr, out - np.asarray(y, dtype=np.float64)


# ---- 2. K = 3 against the oracle ----------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_fused_gradients_match_oracle(gpu_ctx, weighted):
    """Float64, L2, all rows, tree by tree with its own y (and w): test_rowset_gradients_match_oracle's
    bars. Gradient: 2e-10 · Σ_i 2 w_i (|ŷ_i| + |y_i|)|g_i|, from the per-row 1e-10 bar the engine's ŷ
    and ∂ŷ/∂c are held to (tests/test_gradients.py) plus the fp64 sum."""
    T = np.float64
    o = srhip.Options(**NAN_OPS)
    trees = srhip.random_population(80, o, 5, T, seed=45) + hand_trees(o)
    X, Y, W = multi_data(T)
    flat = srhip.flatten(trees, o, dtype=T)
    co = flat.const_off
    tg = cyc(len(trees))
    mds = srhip.MultiDataset(X, Y, weights=W if weighted else None)
    dev = mds.device()
    prog = srhip.Program(dev.ctx, flat, T, interpreted=True)
    s, g, ws, ok = prog.eval_loss_grad_targets(dev, K.LOSS["L2"], tg)
    assert gpu_ctx.last_kernel_name() == "grad_kernel_targets<double>" and gpu_ctx.last_tree_code() == 0
    want_ws = W.astype(np.float64).sum(axis=1) if weighted else np.full(NT, float(N))
    assert np.allclose(ws, want_ws, rtol=1e-12)
    nok = nfail = 0
    for t in range(len(trees)):
        y = Y[tg[t]]
        w = W[tg[t]] if weighted else None
        w64 = np.ones(N) if w is None else w.astype(np.float64)
        rok, out, gr, res = oracle_terms(flat, t, X, y, w)
        assert rok == bool(ok[t]), f"did_succeed of tree {t} differs from the oracle"
        nc = co[t + 1] - co[t]
        if not rok:
            nfail += 1
            assert np.isnan(s[t]) and np.all(np.isnan(g[co[t]:co[t + 1]]))
            continue
        nok += 1
        with np.errstate(all="ignore"):
            ref_sum = np.sum(w64 * res * res)
        if not np.isfinite(ref_sum):
            assert not np.isfinite(s[t]), t
            continue
        sp = loss_spread([trees[t]], o, X, y, w, T)[0]
        assert_close_conditioned(s[t:t + 1], np.array([ref_sum]), np.array([sp]), rtol=1e-9,
                                 msg=f"loss sum of tree {t}")
        if nc:
            gref = 2.0 * (gr @ (w64 * res))
            bar = 2e-10 * np.sum(2.0 * w64 * (np.abs(out) + np.abs(y)) * np.abs(gr), axis=1)
            gt = g[co[t]:co[t + 1]]
            fin = np.isfinite(bar) & np.isfinite(gref)
            err = np.abs(gt[fin] - gref[fin])
            assert np.all(err <= bar[fin]), (t, err, bar)
            assert not np.isfinite(gt[~fin]).any(), (t, gt, gref)
    assert nok >= 30 and nfail >= 5, (nok, nfail)


# ---- 3. K = 3 against the views -----------------------------------------------------------------
def view_bars(T, flat, X, Y, W, tg):
    """Per tree the sum's bar and per constant the gradient's: 2·(16·4 + 6)·ε_T·Σ_i |w_i ℓ_i| and the
    same with |w_i ℓ'_i ∂ŷ_i/∂c| (L2), the sums from the Float64 oracle. Both sides add the same
    per-row terms from the same routines and differ only in how many tiles a lane adds before the
    shuffle tree and the fp64 row-group sum: at most 16 tiles × 4 rows plus 6 shuffle steps a side.
    Also the oracle's did_succeed."""
    co = flat.const_off
    c = 2.0 * (16 * 4 + 6) * EPS[np.dtype(T).type]
    sbar = np.full(flat.ntrees, np.nan)
    gbar = np.full(int(co[-1]), np.nan)
    rok = np.zeros(flat.ntrees, dtype=bool)
    for t in range(flat.ntrees):
        w64 = np.ones(X.shape[1]) if W is None else W[tg[t]].astype(np.float64)
        rok[t], out, gr, res = oracle_terms(flat, t, X, Y[tg[t]], None)
        with np.errstate(all="ignore"):
            sbar[t] = c * np.sum(np.abs(w64 * res * res))
            if co[t + 1] > co[t]:
                gbar[co[t]:co[t + 1]] = c * np.sum(np.abs(w64 * 2.0 * res * gr), axis=1)
    return sbar, gbar, rok


def assert_within(a, b, bar, T, what):
    """|a - b| <= bar; entries whose bar is not finite, or beyond the dtype's largest value / 1e6, by
    finiteness only."""
    a, b, bar = np.asarray(a), np.asarray(b), np.asarray(bar)
    tight = np.isfinite(bar) & (bar <= float(np.finfo(T).max) / 1e6)
    with np.errstate(all="ignore"):
        err = np.abs(a[tight] - b[tight])
    same = (np.isnan(a[tight]) & np.isnan(b[tight])) | (a[tight] == b[tight])  # (a sum that overflowed on both sides)
    bad = ~same & ~(err <= bar[tight])
    assert not bad.any(), (what, np.flatnonzero(tight)[bad], a[tight][bad], b[tight][bad], bar[tight][bad])
    assert np.array_equal(np.isfinite(a[~tight]), np.isfinite(b[~tight])), what


def fused_vs_views(ctx, T, o, trees, X, Y, W, tg, what):
    """The fused call against eval_loss_grad of an interpreted program on each view, under view_bars.
    Returns (fused kernel name, ok, the oracle's did_succeed)."""
    flat = srhip.flatten(trees, o, dtype=T)
    co = flat.const_off
    mds = srhip.MultiDataset(X, Y, weights=W)
    dev = mds.device()
    prog = srhip.Program(dev.ctx, flat, T, interpreted=True)
    s, g, ws, ok = prog.eval_loss_grad_targets(dev, L2.kind, tg, L2.params)
    name = ctx.last_kernel_name()
    assert ctx.last_tree_code() == 0
    sv, gv, okv = np.zeros_like(s), np.zeros_like(g), np.zeros_like(ok)
    per_const = np.repeat(tg, np.diff(co))
    for k in range(Y.shape[0]):
        s1, g1, w1, ok1 = prog.eval_loss_grad(mds.target(k).device(), L2.kind, L2.params)
        assert ws[k] == w1, (what, k)
        sv[tg == k], okv[tg == k] = s1[tg == k], ok1[tg == k]
        gv[per_const == k] = g1[per_const == k]
    assert np.array_equal(ok, okv), (what, np.flatnonzero(ok != okv))
    sbar, gbar, rok = view_bars(T, flat, X, Y, W, tg)
    assert_within(s, sv, sbar, T, what + " sums")
    assert_within(g, gv, gbar, T, what + " gradients")
    assert np.all(np.isnan(s[~ok])) and np.all(np.isnan(g[np.repeat(~ok, np.diff(co))])), what
    return name, ok, rok


def target_patterns(ntrees):
    rng = np.random.default_rng(146)
    return {"random": rng.integers(0, NT, ntrees).astype(np.int32),
            "all-on-2": np.full(ntrees, 2, dtype=np.int32),
            "none-on-1": rng.choice([0, 2], ntrees).astype(np.int32)}


@pytest.mark.parametrize("pattern", ["random", "all-on-2", "none-on-1"])
@pytest.mark.parametrize("T", DTYPES)
def test_fused_gradients_match_views(gpu_ctx, T, pattern):
    T = np.dtype(T).type
    o = srhip.Options(**OPS)
    trees = srhip.random_population(40, o, 5, T, seed=42) + hand_trees(o)
    X, Y, W = multi_data(T)
    tg = target_patterns(len(trees))[pattern]
    for weighted in (False, True):
        name, ok, rok = fused_vs_views(gpu_ctx, T, o, trees, X, Y, W if weighted else None, tg,
                                       f"{tname(T)} {pattern} weighted={weighted}")
        assert name == f"grad_kernel_targets<{tname(T)}>", name
        assert rok.sum() >= 40 and ok.sum() >= 40, (int(rok.sum()), int(ok.sum()))


# ---- 4. wide and boundary -----------------------------------------------------------------------
def boundary_case(ctx, T, nfeat, ntg):
    T = np.dtype(T).type
    o, trees, flat, X, y, w = WC.problem(T, nfeat, 700, 200)
    B = o.make_binary
    # the last feature, read by a tree with constants
    trees = list(trees) + [B("+", B("*", Node(val=0.75), Node(f"x{nfeat}")), Node(val=-0.25))]
    rng = np.random.default_rng(145)
    Y = np.stack([y] + [(y * T(0.5 + k) + X[k]).astype(T) for k in range(1, ntg)])
    Wt = np.stack([w] + [np.abs(rng.standard_normal(700)).astype(T) + T(0.01) for _ in range(1, ntg)])
    tg = rng.integers(0, ntg, len(trees)).astype(np.int32)
    name, ok, rok = fused_vs_views(ctx, T, o, trees, X, Y, Wt, tg, f"{tname(T)} {nfeat} features")
    assert ok[-1] and ok.sum() >= 100, int(ok.sum())
    return name


def test_boundary_f32_75_features_4_weighted_targets(gpu_ctx, monkeypatch):
    """75 features + 4·2 columns = 83 arrays, the shape at which the fused scoring call goes wide
    (tests/test_targets_gpu.py). The gradient kernels' tiles are 256, 128 and 64 rows, not 512, so
    83 arrays still fit in LDS here; the same shape then runs the wide targets variant by
    SRHIP_WIDE=1 (read per call), against views that run wide too."""
    assert boundary_case(gpu_ctx, np.float32, 75, 4) == "grad_kernel_targets<float>"
    monkeypatch.setenv("SRHIP_WIDE", "1")
    assert boundary_case(gpu_ctx, np.float32, 75, 4) == "grad_kernel_wide_targets<float>"


def test_wide_f64_100_features(gpu_ctx, monkeypatch):
    """100 features + 3·2 columns of Float64 (64-row tiles: 53 KiB, fits), then forced wide."""
    assert boundary_case(gpu_ctx, np.float64, 100, 3) == "grad_kernel_targets<double>"
    monkeypatch.setenv("SRHIP_WIDE", "1")
    assert boundary_case(gpu_ctx, np.float64, 100, 3) == "grad_kernel_wide_targets<double>"


def test_wide_f32_650_features_4_weighted_targets(gpu_ctx):
    """650 features + 8 columns: 658 arrays of even the deep variant's 64-row tile are 164.5 KiB, past
    the 160 KiB of LDS, so every pass plans the wide targets variant on its own."""
    assert boundary_case(gpu_ctx, np.float32, 650, 4) == "grad_kernel_wide_targets<float>"


# ---- 5. row sets with targets -------------------------------------------------------------------
@pytest.mark.parametrize("bs", [50, 700])
@pytest.mark.parametrize("T", DTYPES)
def test_rowset_gradients_with_targets_equal_views_bit_for_bit(gpu_ctx, T, bs):
    T = np.dtype(T).type
    o = srhip.Options(**OPS)
    trees = srhip.random_population(40, o, 5, T, seed=42) + hand_trees(o)
    flat = srhip.flatten(trees, o, dtype=T)
    co = flat.const_off
    X, Y, W = multi_data(T)
    tg = cyc(len(trees))
    rows = samples(len(trees), bs)  # (sample 0 is one row repeated)
    per_const = np.repeat(tg, np.diff(co))
    for weighted in (False, True):
        mds = srhip.MultiDataset(X, Y, weights=W if weighted else None)
        dev = mds.device()
        prog = srhip.Program(dev.ctx, flat, T, interpreted=True)
        for loss in (L2, HUBER):
            what = f"{tname(T)} bs={bs} weighted={weighted} {type(loss).__name__}"
            s, g, ws, ok = prog.eval_loss_grad_rowsets_targets(dev, loss.kind, tg, rows, loss.params)
            assert gpu_ctx.last_kernel_name() == f"grad_kernel_seg<{tname(T)}>", what
            assert gpu_ctx.last_tree_code() == 0
            for k in range(NT):
                s1, g1, w1, ok1 = prog.eval_loss_grad_rowsets(mds.target(k).device(), loss.kind, rows, loss.params)
                m, mc = tg == k, per_const == k
                assert np.array_equal(ok[m], ok1[m]), (what, k)
                assert bits_equal(s[m], s1[m]) and bits_equal(g[mc], g1[mc]) and bits_equal(ws[m], w1[m]), (what, k)
            assert ok[:-1].sum() >= 30 and not ok[-1], what


@pytest.mark.parametrize("T", DTYPES)
def test_did_succeed_is_per_sample_and_target(gpu_ctx, T):
    T = np.dtype(T).type
    o = srhip.Options(**NAN_OPS)
    tree = lambda: o.make_unary("safe_sqrt", o.make_binary("*", Node(val=1.0), Node("x1")))
    trees = [tree(), tree()]
    X, Y, W = multi_data(T)
    pos, neg = np.flatnonzero(X[0] > 0), np.flatnonzero(X[0] < 0)
    rng = np.random.default_rng(3)
    rows = np.stack([rng.choice(pos, 50), rng.choice(pos, 50)])
    rows[1, 17] = neg[0]
    tg = np.array([2, 1], dtype=np.int32)
    mds = srhip.MultiDataset(X, Y, weights=W)
    dev = mds.device()
    prog = srhip.Program(dev.ctx, srhip.flatten(trees, o, dtype=T), T, interpreted=True)
    s, g, ws, ok = prog.eval_loss_grad_rowsets_targets(dev, L2.kind, tg, rows)
    assert list(ok) == [True, False]
    assert np.isnan(s[1]) and np.isnan(g[1]) and np.isfinite(s[0]) and np.isfinite(g[0])
    s1, g1, w1, ok1 = prog.eval_loss_grad_rowsets(mds.target(2).device(), L2.kind, rows)
    assert ok1[0] and s[0] == s1[0] and g[0] == g1[0] and ws[0] == w1[0]
    want = 0.0
    for v in W[1].astype(np.float64)[rows[1]]:  # (the library adds the sample's weights in order)
        want += float(v)
    assert ws[1] == want


# ---- 6. the optimiser ---------------------------------------------------------------------------
def noise_offsets(flat, nre):
    return np.concatenate([[0], np.cumsum(nre * np.diff(flat.const_off))])


@pytest.mark.parametrize("bs", [50, 700])
@pytest.mark.parametrize("algorithm", ["BFGS", "NelderMead"])
@pytest.mark.parametrize("T", DTYPES)
def test_rowset_optimiser_with_targets_equals_views_bit_for_bit(gpu_ctx, T, algorithm, bs):
    """Tree t of the fused row-set run == tree t optimised alone on the view of its target with its
    own sample and its slice of the start noise: constants, loss, converged, num_evals."""
    T = np.dtype(T).type
    o, trees = opt_trees(T)
    o.optimizer_algorithm = algorithm
    X, Y, W = multi_data(T)
    wt = W if algorithm == "BFGS" else None  # both weight paths
    tg = cyc(len(trees))
    rows = samples(len(trees), bs, seed=202)
    flat = srhip.flatten(trees, o, dtype=T)
    nre = o.optimizer_nrestarts
    noise = srhip.constant_optimization.start_noise(flat, nre, np.random.default_rng(9))
    noff = noise_offsets(flat, nre)
    mds = srhip.MultiDataset(X, Y, weights=wt)
    mine = [t.copy() for t in trees]
    res = srhip.optimize_constants_batch(mds, mine, o, noise=noise, row_idx=rows, targets=tg, fused=True)
    prof = srhip.constant_optimization.last_profile()
    assert prof["n_segment_evals"] == prof["n_loss"] + prof["n_grad"] > 0
    assert gpu_ctx.last_tree_code() == 0
    assert res.converged.any()
    for t, tree in enumerate(trees):
        alone = [tree.copy()]
        ref = srhip.optimize_constants_batch(mds.target(int(tg[t])), alone, o, noise=noise[noff[t]:noff[t + 1]],
                                             row_idx=rows[t:t + 1])
        what = f"{tname(T)} {algorithm} bs={bs} tree {t}"
        assert bits_equal(np.asarray(srhip.get_constants(mine[t]), dtype=T),
                          np.asarray(srhip.get_constants(alone[0]), dtype=T)), what
        assert np.array_equal(res.losses[t:t + 1], ref.losses, equal_nan=True), (what, res.losses[t], ref.losses)
        assert res.converged[t] == ref.converged[0], what
        assert res.num_evals[t] == ref.num_evals[0], what


@pytest.mark.parametrize("algorithm", ["BFGS", "NelderMead"])
@pytest.mark.parametrize("T", DTYPES)
def test_one_target_optimiser_equals_plain_optimiser_bit_for_bit(gpu_ctx, monkeypatch, T, algorithm):
    """All rows, K = 1, fewer than 256 candidates and no tree code on the plain side: the same
    launches in the same order."""
    monkeypatch.setenv("SRHIP_JIT", "0")
    monkeypatch.setenv("SRHIP_GJIT", "0")
    T = np.dtype(T).type
    o, trees = opt_trees(T)
    o.optimizer_algorithm = algorithm
    assert len(trees) * (1 + o.optimizer_nrestarts) < 256
    X, y, w = data(T)
    flat = srhip.flatten(trees, o, dtype=T)
    noise = srhip.constant_optimization.start_noise(flat, o.optimizer_nrestarts, np.random.default_rng(9))
    for wt in (None, w):
        a, b = [t.copy() for t in trees], [t.copy() for t in trees]
        one = srhip.MultiDataset(X, y[None, :], weights=None if wt is None else wt[None, :])
        ra = srhip.optimize_constants_batch(one, a, o, noise=noise, fused=True)
        pa = srhip.constant_optimization.last_profile()
        rb = srhip.optimize_constants_batch(srhip.Dataset(X, y, weights=wt), b, o, noise=noise)
        pb = srhip.constant_optimization.last_profile()
        assert (pa["n_loss"], pa["n_grad"], pa["n_create"]) == (pb["n_loss"], pb["n_grad"], pb["n_create"])
        assert ra.converged.any()
        for t in range(len(trees)):
            assert bits_equal(np.asarray(srhip.get_constants(a[t]), dtype=T),
                              np.asarray(srhip.get_constants(b[t]), dtype=T)), t
        assert np.array_equal(ra.losses, rb.losses, equal_nan=True)
        assert np.array_equal(ra.converged, rb.converged) and np.array_equal(ra.num_evals, rb.num_evals)


class _Shape:
    def __init__(self, T):
        self.T = T


def structure_key(tree, o, T):
    f = srhip.flatten([tree], o, dtype=T)
    k, a, _ = f.tree(0)
    return np.asarray(k).tobytes() + b"|" + np.asarray(a).tobytes()


@pytest.mark.parametrize("algorithm", ["BFGS", "NelderMead"])
@pytest.mark.parametrize("T", DTYPES)
def test_fused_optimiser_follows_the_reference_driver(gpu_ctx, T, algorithm):
    """All rows, K = 3: tests/constopt_reference.py over an evaluator that scores a candidate set with
    eval_loss_targets / eval_loss_grad_targets and the targets of the candidates' input trees
    reproduces srhip_optimize_constants_targets bit for bit (straggler sets of the line search and
    the simplex programs included: every set the reference makes goes through the factory)."""
    T = np.dtype(T).type
    o, trees = opt_trees(T)
    o.optimizer_algorithm = algorithm
    X, Y, W = multi_data(T)
    # a candidate is a copy of its input tree with other constants: its structure names its target
    key_tg = {}
    for t, tree in enumerate(trees):
        key_tg.setdefault(structure_key(tree, o, T), t % NT)
    tg = np.array([key_tg[structure_key(tree, o, T)] for tree in trees], dtype=np.int32)
    assert len(set(tg)) == NT
    mds = srhip.MultiDataset(X, Y, weights=W)
    dev = mds.device()
    nsets = []

    class Evaluator:
        def __init__(self, cands):
            self.tg = np.array([key_tg[structure_key(c, o, T)] for c in cands], dtype=np.int32)
            self.flat = srhip.flatten(cands, o, dtype=T)
            self.prog = srhip.Program(dev.ctx, self.flat, T, interpreted=True, varying_constants=True)
            nsets.append(len(cands))

        def loss_grad(self, consts):
            self.prog.set_constants(np.asarray(consts, dtype=T))
            s, g, ws, ok = self.prog.eval_loss_grad_targets(dev, L2.kind, self.tg)
            w = ws[self.tg]
            with np.errstate(all="ignore"):
                f = s / w
                gg = g / np.repeat(w, np.diff(self.flat.const_off))
            gg[np.repeat(~ok, np.diff(self.flat.const_off))] = np.nan
            return np.where(ok & np.isfinite(f), f, np.inf), gg

        def loss_only(self, consts):
            self.prog.set_constants(np.asarray(consts, dtype=T))
            s, ws, ok = self.prog.eval_loss_targets(dev, L2.kind, self.tg)
            with np.errstate(all="ignore"):
                f = s / ws[self.tg]
            return np.where(ok & np.isfinite(f), f, np.inf)

    flat = srhip.flatten(trees, o, dtype=T)
    noise = srhip.constant_optimization.start_noise(flat, o.optimizer_nrestarts, np.random.default_rng(9))
    a, b = [t.copy() for t in trees], [t.copy() for t in trees]
    ra = srhip.optimize_constants_batch(mds, a, o, noise=noise, targets=tg, fused=True)
    prof = srhip.constant_optimization.last_profile()
    assert prof["n_segment_evals"] == 0 and prof["n_loss"] > 0 and gpu_ctx.last_tree_code() == 0
    rb = REF.optimize_constants_batch(_Shape(T), b, o, noise, Evaluator)
    # the library made straggler sets of its line searches / simplex points besides the candidates'
    # and the final set; the reference keeps every candidate in one evaluator (or several sizes of its own)
    assert prof["n_create"] > 2 and len(set(nsets)) >= 2
    assert ra.converged.any()
    for t in range(len(trees)):
        assert bits_equal(np.asarray(srhip.get_constants(a[t]), dtype=T),
                          np.asarray(srhip.get_constants(b[t]), dtype=T)), t
    assert np.array_equal(ra.losses, np.asarray(rb.losses, dtype=T).astype(np.float64), equal_nan=True)
    assert np.array_equal(ra.converged, rb.converged) and np.array_equal(ra.num_evals, rb.num_evals)


@pytest.mark.parametrize("T", [pytest.param(np.float64, id="f64"), pytest.param(np.float32, id="f32")])
def test_fused_optimiser_recovers_each_targets_constants(gpu_ctx, T):
    """c1·cos(x4) + c2·x1·x1 + c3, one tree per target, Y_k = a_k·cos(x4) + b_k·x1² + d_k: one fused
    call, every tree to its own target's constants (test_engine_optimizer_matches_oracle_driver's atol).
    Whether a Float32 run of 8 iterations ends converged depends on its start, so the three problems
    are (2, 1, -2) scaled by 1, -2 and 1/2 with x0 and the start noise scaled alike: the three
    trajectories are then the same up to powers of two, and a tree that went to another target's
    column would end at that target's constants."""
    T = np.dtype(T).type
    o = srhip.Options(**OPS)
    B, U = o.make_binary, o.make_unary
    tree = lambda: B("+", B("+", B("*", Node(val=1.0), U("cos", Node("x4"))),
                            B("*", Node(val=0.5), B("*", Node("x1"), Node("x1")))), Node(val=0.0))
    X, _, _ = data(T)
    scale = np.array([1.0, -2.0, 0.5])
    abd = scale[:, None] * np.array([2.0, 1.0, -2.0])
    Y = np.stack([a * np.cos(X[3]) + b * X[0] * X[0] + d for a, b, d in abd]).astype(T)
    trees = [tree() for _ in range(NT)]
    for t, k in enumerate([2, 0, 1]):
        srhip.set_constants(trees[t], [T(scale[k] * c) for c in srhip.get_constants(trees[t])])
    one = srhip.constant_optimization.start_noise(srhip.flatten(trees, o, dtype=T), o.optimizer_nrestarts,
                                                  np.random.default_rng(0))[6:12]
    mds = srhip.MultiDataset(X, Y)
    res = srhip.optimize_constants_batch(mds, trees, o, noise=np.tile(one, NT), targets=[2, 0, 1], fused=True)
    atol = 1e-6 if T == np.float64 else 2e-3
    assert res.converged.all()
    for t, k in enumerate([2, 0, 1]):
        assert np.allclose(srhip.get_constants(trees[t]), abd[k], atol=atol), (t, srhip.get_constants(trees[t]))
    assert np.all(res.losses < (1e-10 if T == np.float64 else 1e-5))
    prof = srhip.constant_optimization.last_profile()
    assert prof["n_grad"] > 0 and prof["n_segment_evals"] == 0 and gpu_ctx.last_tree_code() == 0


# ---- 7. rules -----------------------------------------------------------------------------------
def test_rules(gpu_ctx):
    T = np.float32
    o = srhip.Options(**OPS)
    trees = hand_trees(o)[:3]
    X, Y, W = multi_data(T)
    mds = srhip.MultiDataset(X, Y, weights=W)
    dev = mds.device()
    flat = srhip.flatten(trees, o, dtype=T)
    prog = srhip.Program(dev.ctx, flat, T, interpreted=True)
    nc = int(flat.const_off[-1])
    lib = srhip._lib.lib()
    INV, UNS = srhip._lib.ERR_INVALID, srhip._lib.ERR_UNSUPPORTED
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rows = np.zeros((3, 4), dtype=np.int64)
    mark = 7.5

    def outs():
        return np.full(3, mark), np.full(nc, mark), np.full(3, mark), np.full(3, 9, dtype=np.uint8)

    def untouched(s, g, ws, ok):
        return np.all(s == mark) and np.all(g == mark) and np.all(ws == mark) and np.all(ok == 9)

    good = np.array([0, 1, 2], dtype=np.int32)
    for tg in (None, np.array([0, 3, 1], dtype=np.int32), np.array([0, -1, 1], dtype=np.int32)):
        tp = None if tg is None else p(tg)
        s, g, ws, ok = outs()
        assert lib.srhip_eval_loss_grad_targets(dev.handle, prog.handle, 0, None, tp, p(s), p(g), p(ws), p(ok)) == INV
        assert untouched(s, g, ws, ok)
        assert lib.srhip_eval_loss_grad_rowsets_targets(dev.handle, prog.handle, 0, None, tp, p(rows), 4, p(s), p(g),
                                                        p(ws), p(ok)) == INV
        assert untouched(s, g, ws, ok)
        with pytest.raises((srhip.SrhipError, ValueError)):
            srhip.optimize_constants_batch(mds, [t.copy() for t in trees], o, rng=np.random.default_rng(0),
                                           targets=tg, fused=True)
    # the optimiser's C entry: a null and an out-of-range target, outputs untouched
    noise = srhip.constant_optimization.start_noise(flat, 2, np.random.default_rng(0))
    opts = srhip._lib.ConstOptOptions(0, 8, 2, 0, None, noise.ctypes.data_as(C.POINTER(C.c_double)), 0)
    consts = np.ascontiguousarray(flat.consts, dtype=T)
    tr = srhip.engine._trees_struct(flat, consts)
    oc, ol, ok8, on = np.full(nc, mark, dtype=T), np.full(3, mark), np.full(3, 9, dtype=np.uint8), np.full(3, mark)
    bad = np.array([0, 3, 1], dtype=np.int32)
    for tp, ri, bs in ((None, None, 0), (p(bad), None, 0), (p(good), p(rows), 0), (p(good), p(rows), -1),
                       (p(good), None, -1)):
        rc = lib.srhip_optimize_constants_targets(dev.ctx.handle, dev.handle, C.byref(tr), C.byref(opts), tp, ri, bs,
                                                  p(oc), p(ol), p(ok8), p(on))
        assert rc == INV, (tp, ri, bs)
        assert np.all(oc == T(mark)) and np.all(ol == mark) and np.all(ok8 == 9) and np.all(on == mark)
    # a negative batch size for the gradient call
    s, g, ws, ok = outs()
    assert lib.srhip_eval_loss_grad_rowsets_targets(dev.handle, prog.handle, 0, None, p(good), p(rows), -1, p(s), p(g),
                                                    p(ws), p(ok)) == INV
    assert untouched(s, g, ws, ok)
    # an expression loss: UNSUPPORTED from all three calls, correct on a view
    lo = loss_options()
    el = srhip.ExprLoss(e4(lo), lo)
    umds = srhip.MultiDataset(X, Y)
    udev = umds.device()
    with pytest.raises(srhip.SrhipError) as e:
        prog.eval_loss_grad_targets(udev, el.kind, good, el.params)
    assert e.value.code == UNS
    with pytest.raises(srhip.SrhipError) as e:
        prog.eval_loss_grad_rowsets_targets(udev, el.kind, good, rows, el.params)
    assert e.value.code == UNS
    eopts = srhip._lib.ConstOptOptions(0, 8, 2, int(el.kind), None, noise.ctypes.data_as(C.POINTER(C.c_double)), 0)
    assert lib.srhip_optimize_constants_targets(udev.ctx.handle, udev.handle, C.byref(tr), C.byref(eopts), p(good),
                                                None, 0, p(oc), p(ol), p(ok8), p(on)) == UNS
    sv, gv, wv, okv = prog.eval_loss_grad(umds.target(1).device(), el.kind, el.params)
    s0, g0, w0, ok0 = prog.eval_loss_grad(srhip.Dataset(X, Y[1]).device(), el.kind, el.params)
    assert okv.any() and np.array_equal(okv, ok0) and bits_equal(sv, s0) and bits_equal(gv, g0)
    # the single-target entry points still refuse the multi-target dataset
    with pytest.raises(srhip.SrhipError) as e:
        prog.eval_loss_grad(dev, 0)
    assert e.value.code == INV and "view" in str(e.value)
    rc = lib.srhip_optimize_constants_batch(dev.ctx.handle, dev.handle, C.byref(tr), C.byref(opts), p(oc), p(ol),
                                            p(ok8), p(on))
    assert rc == INV and b"view" in lib.srhip_last_error()
    # a program of more features than the dataset
    small = srhip.MultiDataset(X[:3], Y)
    with pytest.raises(srhip.SrhipError) as e:
        prog.eval_loss_grad_targets(small.device(), 0, good)
    assert e.value.code == INV and "feature" in str(e.value)
    rc = lib.srhip_optimize_constants_targets(dev.ctx.handle, small.device().handle, C.byref(tr), C.byref(opts),
                                              p(good), None, 0, p(oc), p(ol), p(ok8), p(on))
    assert rc == INV
    # an empty tree list
    l, gl, okl = srhip.eval_loss_grad_batch([], mds, o, targets=[], fused=True)
    assert l.shape == (0,) and gl == [] and okl.shape == (0,)
    r = srhip.optimize_constants_batch(mds, [], o, rng=np.random.default_rng(0), targets=[], fused=True)
    assert r.losses.shape == (0,)


# ---- 8. the public functions --------------------------------------------------------------------
@pytest.mark.parametrize("T", DTYPES)
def test_public_functions_fused_and_views_agree(gpu_ctx, T):
    T = np.dtype(T).type
    o = srhip.Options(**OPS)
    trees = srhip.random_population(40, o, 5, T, seed=42) + hand_trees(o)
    X, Y, W = multi_data(T)
    tg = cyc(len(trees))
    mds = srhip.MultiDataset(X, Y, weights=W)
    flat = srhip.flatten(trees, o, dtype=T)
    co = flat.const_off
    lf, gf, okf = srhip.eval_loss_grad_batch(trees, mds, o, targets=tg, fused=True)
    lv, gv, okv = srhip.eval_loss_grad_batch(trees, mds, o, targets=tg, fused=False)
    assert np.array_equal(okf, okv) and okf.sum() >= 40
    sbar, gbar, _ = view_bars(T, flat, X, Y, W, tg)
    wsum = W.astype(np.float64).sum(axis=1)[tg]
    # (the losses are rounded to T after the division: one more rounding each)
    assert_within(lf.astype(np.float64), lv.astype(np.float64),
                  sbar / wsum + 2 * EPS[T] * np.abs(lv.astype(np.float64)), T, "losses")
    for t in range(len(trees)):
        assert_within(gf[t], gv[t], gbar[co[t]:co[t + 1]] / wsum[t], T, f"gradient of tree {t}")
    # row sets: bit for bit
    rows = samples(len(trees), 50)
    lf, gf, okf = srhip.eval_loss_grad_batch(trees, mds, o, row_idx=rows, targets=tg, fused=True)
    lv, gv, okv = srhip.eval_loss_grad_batch(trees, mds, o, row_idx=rows, targets=tg, fused=False)
    assert np.array_equal(okf, okv) and bits_equal(lf, lv)
    assert all(bits_equal(a, b) for a, b in zip(gf, gv))
    # the optimiser on row sets, both paths: the same trees, updated in place
    oo, otrees = opt_trees(T)
    otg = cyc(len(otrees))
    orows = samples(len(otrees), 50, seed=202)
    noise = srhip.constant_optimization.start_noise(srhip.flatten(otrees, oo, dtype=T), oo.optimizer_nrestarts,
                                                    np.random.default_rng(9))
    a, b = [t.copy() for t in otrees], [t.copy() for t in otrees]
    ra = srhip.optimize_constants_batch(mds, a, oo, noise=noise, row_idx=orows, targets=otg, fused=True)
    rb = srhip.optimize_constants_batch(mds, b, oo, noise=noise, row_idx=orows, targets=otg, fused=False)
    assert ra.converged.any() and np.array_equal(ra.converged, rb.converged)
    assert np.array_equal(ra.losses, rb.losses, equal_nan=True) and np.array_equal(ra.num_evals, rb.num_evals)
    changed = 0
    for t in range(len(otrees)):
        ca, cb, c0 = (np.asarray(srhip.get_constants(x[t]), dtype=T) for x in (a, b, otrees))
        assert bits_equal(ca, cb), t
        changed += int(not bits_equal(ca, c0))
    assert changed > 0
