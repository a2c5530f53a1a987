"""Every interpreter kernel variant against the oracle, by construction.

eval_kernel and grad_kernel are matrices of template instantiations chosen on
the host: {Float32, Float64} x {shallow BASIC, shallow FULL, deep} x {L2, generic
loss, per-row outputs} x {weighted, not} for evaluation, and x tangents G in
{1, 2, 4} x {per-row gradients, loss gradients} for gradients. Which cell a tree
reaches follows from its stack need (compile.cpp compute_need: an operator over
two leaves needs 0 slots, an operator over two subtrees of equal need one more),
its instruction count, its number of constants and the batch's operators. The
families below are built so that each must land in one cell;
Program.pass_info() says where they landed and is asserted, so a change of the
routing rules that moves a family fails here instead of silently leaving a cell
untested. Batches stay far below the tree-code bar: everything is interpreted.

All trees use + - * (and relu / max in the FULL family): the predictions are
bit-exact by the project's own bar, so every kink and the ZeroOne step fall on
the same side in the engine and in the checker and no bound needs a spread
allowance. Bounds:

  per-row outputs   bit-identical to the oracle's in T
  distance losses   |got - ref| <= rtol·|ref|, rtol = 1e-5 (Float32), 1e-9 (Float64)
  margin losses     check_sums of test_margin_losses_gpu.py, unchanged
  loss gradients    rtol·Σ|terms| + DV + 1e-30 (test_jit_losses_gpu.py)
  per-row gradients Float64: rtol = atol = 1e-10 (values 1e-12), as
                    test_gradients.test_many_constants_and_deep_trees;
                    Float32: see check_grad_out

Features are uniform in [-1.2, 1.2] and constants in [-1, 1]: checked on the CPU
with the oracle, every tree of every family succeeds in both dtypes at every n
used (asserted as exact counts below); on the planted data of the failure test
exactly the four overflow trees fail.
"""
import contextlib
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import margin_reference as M
import oracle
import srhip
from srhip import Node
from srhip import constants as K
from test_jit_losses_gpu import _dloss
from test_margin_losses_gpu import LOSSES as MARGIN_LOSSES
from test_margin_losses_gpu import RTOL, check_sums, margin_seed, reference_sums

pytestmark = pytest.mark.gpu

ADD, SUB, MUL, MAX = 1, 2, 3, 4  # indices into OPS' binary operators
RELU = 1
LO, HI, PLANT = -1.2, 1.2, 2.4  # the feature range, and the planted largest |x|
NFEAT = 5
KGRADG = 4  # tangents of a gradient work item (srhip_internal.h kGradG)

FAMILIES = ["shallow-basic", "shallow-full", "deep-eval", "long-chain", "grad-deep", "grad-need4", "constants"]
DTYPES = [np.float32, np.float64]
CELLS = [pytest.param(f, T, id=f"{f}-{np.dtype(T).name}") for f in FAMILIES for T in DTYPES]

MARGIN_KINDS = {K.LOSS[n] for n in M.NAMES}
LOSS_NAME = {v: k for k, v in K.LOSS.items()}
L2, HUBER, LOGITDIST = srhip.L2DistLoss(), srhip.HuberLoss(0.8), srhip.LogitDistLoss()
# all eleven margin losses, and the two parametric ones at a second parameter
LOSS_CELLS = [L2, HUBER, LOGITDIST] + list(MARGIN_LOSSES) + [srhip.SmoothedL1HingeLoss(2.0), srhip.DWDMarginLoss(3.0)]
GRAD_CELLS = [L2, HUBER, LOGITDIST, srhip.L1HingeLoss(), srhip.LogitMarginLoss(), srhip.ModifiedHuberLoss(),
              srhip.DWDMarginLoss(1.0)]


def lname(loss):
    return f"{LOSS_NAME[loss.kind]}({loss.param:g})"


@functools.lru_cache(maxsize=None)
def opts():
    return srhip.Options(binary_operators=["+", "-", "*", "max"], unary_operators=["relu"])


# ---- tree families ---------------------------------------------------------------

def _pair(rng, const):
    """An operator over two leaves: two different features, or a feature and a constant
    (so every subtree holds a feature and nothing folds)."""
    f = rng.choice(NFEAT, 2, replace=False) + 1
    a = Node(feature=int(f[0]))
    b = Node(val=float(rng.uniform(0.25, 1.0) * rng.choice([-1.0, 1.0]))) if const else Node(feature=int(f[1]))
    if rng.random() < 0.5:
        a, b = b, a
    return Node(int(rng.integers(ADD, MUL + 1)), a, b)


def balanced(rng, depth, nconst):
    """`depth` levels of + - * over 2^depth leaves, `nconst` of them constants: stack need depth - 1."""
    npairs = 2 ** (depth - 1)
    withc = set(rng.choice(npairs, nconst, replace=False).tolist())
    level = [_pair(rng, i in withc) for i in range(npairs)]
    while len(level) > 1:
        level = [Node(int(rng.integers(ADD, MUL + 1)), level[i], level[i + 1]) for i in range(0, len(level), 2)]
    return level[0]


def comb(rng, nops, nconst):
    """((x ∘ leaf) ∘ leaf) ∘ ...: nops instructions, stack need 0."""
    withc = set(rng.choice(nops, nconst, replace=False).tolist())
    t = Node(feature=int(rng.integers(1, NFEAT + 1)))
    for i in range(nops):
        leaf = (Node(val=float(rng.uniform(0.25, 1.0) * rng.choice([-1.0, 1.0]))) if i in withc
                else Node(feature=int(rng.integers(1, NFEAT + 1))))
        t = Node(int(rng.choice([ADD, SUB, MUL], p=[0.4, 0.4, 0.2])), t, leaf)
    return t


def terms(rng, k):
    """A chain of k (feature ∘ constant) terms: exactly k constants, stack need at most 1."""
    t = _pair(rng, True)
    for _ in range(k - 1):
        t = Node(int(rng.integers(ADD, MUL + 1)), t, _pair(rng, True))
    return t


CONSTANT_COUNTS = [1, 2, 3, 4, 5, 6, 8, 9]


@functools.lru_cache(maxsize=None)
def family(name):
    """(trees, need per tree): fixed seed per family."""
    rng = np.random.default_rng(7000 + FAMILIES.index(name))
    if name == "shallow-basic":
        shape = [(1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (3, 4), (3, 1)]
    elif name == "shallow-full":
        shape = [(2, 1), (2, 2), (3, 1), (3, 2), (3, 3), (3, 4)]
    elif name == "deep-eval":
        shape = [(4, 1), (4, 2), (4, 4), (6, 3), (6, 5), (6, 2)]
    elif name == "grad-deep":
        shape = [(6, 5), (6, 9), (6, 5), (7, 9), (7, 5), (7, 9)]
    elif name == "grad-need4":
        shape = [(5, k) for k in (1, 2, 3, 4, 5, 6)]
    elif name == "long-chain":
        return [comb(rng, nops, k) for nops, k in [(70, 1), (72, 2), (80, 3), (96, 4), (75, 5), (70, 2)]], [0] * 6
    else:
        assert name == "constants"
        return [terms(rng, k) for k in CONSTANT_COUNTS], [0] + [1] * (len(CONSTANT_COUNTS) - 1)
    trees = [balanced(rng, d, k) for d, k in shape]
    if name == "shallow-full":  # one relu or max in each tree
        for i, t in enumerate(trees):
            if i % 2:
                t.op = MAX
            else:
                t.l = Node(RELU, t.l)
    return trees, [d - 1 for d, _ in shape]


def expected_grad_items(name):
    """Work items per pass (G = 1, 2, 4, deep) by the rule of the gradient programs: one item per
    group of up to kGradG constants, in the pass of its tangent count, or the deep pass when the
    tree needs more than 4 stack slots."""
    trees, need = family(name)
    items = [0, 0, 0, 0]
    for t, nd in zip(trees, need):
        nc = len(srhip.get_constants(t))
        for g0 in range(0, nc, KGRADG):
            ntan = min(KGRADG, nc - g0)
            items[3 if nd > 4 else 0 if ntan <= 1 else 1 if ntan <= 2 else 2] += 1
    return tuple(items)


def eval_is_deep(name):
    return name not in ("shallow-basic", "shallow-full", "constants")


def eval_tile(T, deep):
    """64·R of the evaluation variant (kernels.hip variant_R)."""
    return 64 * ((4 if deep else 8) if T == np.float32 else (2 if deep else 4))


def grad_tiles(T, name):
    """64·R of every gradient pass the family reaches (grad_kernels.hip grad_R)."""
    out = set()
    for k, cnt in enumerate(expected_grad_items(name)):
        if cnt:
            out.add(64 * (1 if (T != np.float32 or k == 3) else 4 if k <= 1 else 2))
    return sorted(out)


def row_counts(tiles):
    """1, around every tile, and two row groups with the second a lone partial tile."""
    ns = {1, 8192 + max(tiles) + 1}
    for t in tiles:
        ns |= {t - 1, t, t + 1}
    return sorted(ns)


def big_n(T, name):
    return 8192 + eval_tile(T, eval_is_deep(name)) + 1


# ---- data and references (computed once per shape, shared, never written to) --------

def overflow_trees(name, T):
    """x1·c and x2·c, alone and added to a tree of the family (so that one fails in the
    family's own kernel variant): c·1.2 is finite in T, c·2.4 is not."""
    c = float(np.finfo(T).max) / 2
    fam = family(name)[0]
    alone = [Node(MUL, Node(feature=f), Node(val=c)) for f in (1, 2)]
    return alone + [Node(ADD, fam[i].copy(), Node(MUL, Node(feature=f), Node(val=c))) for i, f in ((0, 1), (1, 2))]


@functools.lru_cache(maxsize=None)
def problem(name, T, n, planted=False):
    T = np.dtype(T).type
    trees = list(family(name)[0])
    nfam = len(trees)
    if planted:
        trees += overflow_trees(name, T)
    flat = srhip.flatten(trees, opts(), dtype=T)
    rng = np.random.default_rng(9000 + n)
    X = rng.uniform(LO, HI, (NFEAT, n))
    if planted:
        X[0, n - 1] = PLANT  # the last valid row of the second row group
        X[1, 0] = PLANT
    X = X.astype(T)
    y = (2 * np.cos(X[3]) + X[0] * X[0] - 2).astype(T)
    ym = np.where(y >= 0, 1, -1).astype(T)
    w = np.abs(rng.standard_normal(n)).astype(T)
    with np.errstate(all="ignore"):
        yhat, ok = oracle.eval_trees(flat, X, dtype=T)
        grads = {}
        for t in np.flatnonzero(ok):
            k, ar, c = flat.tree(t)
            yh, gc, okt = oracle.eval_grad_consts(k, ar, c.astype(T), X, len(c), dtype=T)
            assert okt and np.array_equal(yh, yhat[t])
            grads[int(t)] = gc.astype(np.float64)
    for a in (X, y, ym, w, yhat, ok):
        a.setflags(write=False)
    return SimpleNamespace(name=name, T=T, n=n, nfam=nfam, trees=trees, flat=flat, X=X, y=y, ym=ym, w=w, yhat=yhat,
                           ok=ok, grads=grads)


class Worst:
    """Worst err/bound per group of cells."""

    def __init__(self):
        self.v = {}

    def add(self, group, err, bound):
        err, bound = np.atleast_1d(err), np.atleast_1d(bound)
        if err.size:
            with np.errstate(all="ignore"):
                r = float(np.max(np.where(err == 0, 0.0, err / bound)))
            self.v[group] = max(self.v.get(group, 0.0), r)

    def line(self, what):
        return f"{what}: worst err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in self.v.items())


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def dataset(ctx, P, loss, weighted):
    return srhip.DeviceDataset(ctx, P.X, P.ym if loss.kind in MARGIN_KINDS else P.y, P.w if weighted else None)


def loss_reference(P, loss, weighted):
    """(Σ w·ℓ per tree in float64, the bound's magnitude Σ w|ℓ|)."""
    w = P.w if weighted else None
    if loss.kind in MARGIN_KINDS:
        return reference_sums(loss, P.yhat, P.ym, w)
    with np.errstate(all="ignore"):
        sums, _, rok = oracle.eval_loss_batch(P.flat, P.X, P.y, w, loss.kind,
                                              loss.params if loss.params is not None else (0.0,), dtype=P.T)
    assert np.array_equal(rok, P.ok)
    return sums, np.abs(sums)  # distance losses are non-negative: Σ w|ℓ| = |Σ w·ℓ|


def check_loss_sums(got, ok, wsum, P, loss, weighted, worst, group, what):
    """did_succeed as the oracle's, failed trees NaN, every other tree within the bound. Returns the
    bound per tree."""
    T, eps = P.T, float(np.finfo(P.T).eps)
    ok = np.asarray(ok).astype(bool)
    assert np.array_equal(ok, P.ok), what
    assert np.isnan(got[~ok]).all(), (what, got[~ok])
    assert wsum == pytest.approx(float(P.w.astype(np.float64).sum() if weighted else P.n), rel=1e-6)
    ref, mag = loss_reference(P, loss, weighted)
    fin = ok & np.isfinite(ref)
    if loss.kind in MARGIN_KINDS:
        with contextlib.redirect_stdout(None):
            check_sums(got, ref, mag, wsum, ok, T, what)
        bound = RTOL[np.dtype(T)] * mag + 4 * eps * wsum
        if loss.kind == K.LOSS["ZEROONE"] and not weighted:
            assert np.array_equal(got[ok], ref[ok]), what  # integer counts, exactly
    else:
        bound = RTOL[np.dtype(T)] * mag
        assert np.isfinite(ref[ok]).all(), what
        err = np.abs(got[fin] - ref[fin])
        assert np.all(err <= bound[fin]), (what, np.flatnonzero(fin)[~(err <= bound[fin])], err, bound[fin])
    worst.add(group, np.abs(got[fin] - ref[fin]), bound[fin])
    return bound


def seed_and_move(P, loss, t):
    """dℓ/dŷ of tree t's rows in float64, and its move under 4 ulp of the loss's argument."""
    eps = float(np.finfo(P.T).eps)
    with np.errstate(all="ignore"):
        if loss.kind in MARGIN_KINDS:
            a = P.yhat[t] * P.ym  # in T
            seed = margin_seed(loss, a, P.ym)
            d = (4 * eps * np.abs(a.astype(np.float64))).astype(P.T)
            return seed, np.maximum(np.abs(margin_seed(loss, a + d, P.ym) - seed),
                                    np.abs(margin_seed(loss, a - d, P.ym) - seed))
        f = (lambda r: 2.0 * r) if loss.kind == K.LOSS["L2"] else (lambda r: _dloss(loss, r))
        r = (P.yhat[t] - P.y).astype(np.float64)  # the residual in T, promoted
        d = 4 * eps * (np.abs(P.yhat[t].astype(np.float64)) + np.abs(P.y.astype(np.float64)))
        return f(r), np.maximum(np.abs(f(r + d) - f(r)), np.abs(f(r - d) - f(r)))


def check_loss_grads(g, P, loss, weighted, worst, what):
    """Every constant's Σ w·ℓ'·∂ŷ/∂c against the oracle's ∂ŷ/∂c in T; NaN for failed trees."""
    rtol = RTOL[np.dtype(P.T)]
    w64 = P.w.astype(np.float64) if weighted else np.ones(P.n)
    co = P.flat.const_off
    checked = 0
    for t in range(P.flat.ntrees):
        lo, hi = co[t], co[t + 1]
        if not P.ok[t]:
            assert hi > lo and np.isnan(g[lo:hi]).all(), (what, t, g[lo:hi])
            continue
        gc = P.grads[t]
        seed, move = seed_and_move(P, loss, t)
        with np.errstate(all="ignore"):
            term = w64 * seed * gc
            dv = move * np.abs(w64 * gc)
        S, G, DV = np.abs(term).sum(axis=1), term.sum(axis=1), dv.sum(axis=1)
        sel = np.isfinite(S) & (S < 1e20)
        with np.errstate(invalid="ignore"):
            err = np.abs(g[lo:hi] - G)
        bound = rtol * S + DV + 1e-30
        assert np.all(err[sel] <= bound[sel]), (what, t, err[sel].tolist(), bound[sel].tolist())
        assert not np.isfinite(g[lo:hi][~sel & ~np.isfinite(G)]).any(), (what, t)
        worst.add("grad", err[sel], bound[sel])
        checked += int(sel.sum())
    return checked


def assert_eval_cell(prog, name, ntrees):
    """The evaluation lists, known once the program is built (before any launch)."""
    info = prog.pass_info()
    assert info["tree_code"] == 0, info
    if eval_is_deep(name):
        assert (info["shallow"], info["deep"]) == (0, ntrees), (name, info)
    else:
        assert (info["shallow"], info["deep"]) == (ntrees, 0), (name, info)
        assert info["opset"] == ("FULL" if name == "shallow-full" else "BASIC"), (name, info)
    assert info["grad_items"] == (0, 0, 0, 0) and info["grad_rest"] == (0, 0, 0, 0), info  # no gradient call yet
    return info


def assert_grad_cell(prog, name):
    info = prog.pass_info()
    exp = expected_grad_items(name)
    assert info["grad_items"] == exp, (name, info, exp)
    assert info["grad_rest"] == (0, 0, 0, 0), info  # no gradient tree code
    assert info["grad_opset"] == ("FULL" if name == "shallow-full" else "BASIC"), (name, info)
    if name == "grad-deep":
        assert exp[:3] == (0, 0, 0) and exp[3] > len(family(name)[0])  # several groups per tree, all deep
    if name == "grad-need4":
        assert exp[3] == 0 and min(exp[:3]) > 0
    if name == "long-chain":
        assert exp[3] == 0  # deep for evaluation by length only
    if name == "constants":  # 5 -> G=4 + G=1, 6 -> G=4 + G=2, 8 -> 2 G=4, 9 -> 2 G=4 + G=1
        assert exp == (3, 2, 8, 0)
    return info


# ---- the cells -------------------------------------------------------------------

@pytest.mark.parametrize("name,T", CELLS)
def test_outputs_and_losses(gpu_ctx, name, T):
    """eval_kernel: per-row outputs (MODE_OUT) bit-identical to the oracle's, and L2 (the compiled
    epilogue), Huber, LogitDist and the margin losses (the generic epilogue), weighted and not, at
    n = 1, T0 - 1, T0, T0 + 1 and 8192 + T0 + 1 of the family's variant."""
    ctx = gpu_ctx
    trees = family(name)[0]
    ns = row_counts([eval_tile(T, eval_is_deep(name))])
    prog = srhip.Program(ctx, problem(name, T, ns[0]).flat, T)
    info = assert_eval_cell(prog, name, len(trees))
    worst = Worst()
    for n in ns:
        P = problem(name, T, n)
        assert int(P.ok.sum()) == len(trees)  # the oracle's success count: every tree, at every n
        out, ok = prog.eval_tree_array(srhip.DeviceDataset(ctx, P.X, P.y))
        assert ctx.last_tree_code() == 0
        assert np.array_equal(ok, P.ok)
        uint = np.uint32 if T == np.float32 else np.uint64
        assert np.array_equal(out.view(uint), P.yhat.view(uint)), (name, n, np.argwhere(out != P.yhat)[:5])
        for weighted in (False, True):
            for loss in LOSS_CELLS:
                what = f"{name} {np.dtype(T).name} {lname(loss)} n={n} weighted={weighted}"
                s, wsum, ok = prog.eval_loss(dataset(ctx, P, loss, weighted), loss.kind, loss.params)
                assert ctx.last_tree_code() == 0, what
                check_loss_sums(s, ok, wsum, P, loss, weighted, worst,
                                "margin" if loss.kind in MARGIN_KINDS else "distance", what)
    print(worst.line(f"{name} {np.dtype(T).name} n={ns} {info}"))


@pytest.mark.parametrize("name,T", CELLS)
def test_loss_gradients(gpu_ctx, name, T):
    """grad_kernel GRAD_LOSS, weighted and not: ∂L/∂c of L2, Huber, LogitDist, L1Hinge (kink),
    LogitMargin, ModifiedHuber (piecewise) and DWDMargin (parametric) against the oracle, around the
    tile of every gradient pass the family reaches; and the loss the gradient call returns against
    the loss call's (a tree of 5, 6 or 9 constants is several work items, of which one writes it)."""
    ctx = gpu_ctx
    ns = row_counts(grad_tiles(T, name))
    prog = srhip.Program(ctx, problem(name, T, ns[0]).flat, T)
    worst = Worst()
    checked = 0
    for n in ns:
        P = problem(name, T, n)
        assert int(P.ok.sum()) == P.flat.ntrees
        for weighted in (False, True):
            for loss in GRAD_CELLS:
                what = f"{name} {np.dtype(T).name} grad {lname(loss)} n={n} weighted={weighted}"
                ds = dataset(ctx, P, loss, weighted)
                sg, g, wsum, okg = prog.eval_loss_grad(ds, loss.kind, loss.params)
                assert ctx.last_tree_code() == 0, what
                bound = check_loss_sums(sg, okg, wsum, P, loss, weighted, worst, "grad-call loss", what)
                s, _, ok = prog.eval_loss(ds, loss.kind, loss.params)
                both = np.isfinite(s) & np.isfinite(sg)
                assert np.array_equal(s[~both], sg[~both], equal_nan=True), what
                assert np.all(np.abs(sg[both] - s[both]) <= bound[both]), (what, sg, s)
                worst.add("grad-call loss vs loss call", np.abs(sg[both] - s[both]), bound[both])
                checked += check_loss_grads(g, P, loss, weighted, worst, what)
    info = assert_grad_cell(prog, name)
    assert checked >= 0.9 * len(ns) * 2 * len(GRAD_CELLS) * int(P.flat.const_off[-1]), checked
    print(worst.line(f"{name} {np.dtype(T).name} n={ns} {info}"))


def abs_tree(t):
    """The tree with `-` turned into `+` and every constant into its absolute value: on |X| its value
    and its ∂/∂c are the sums of the absolute values of the terms of the tree's value and ∂ŷ/∂c."""
    if t.degree == 0:
        return Node(val=abs(t.val)) if t.constant else Node(feature=t.feature)
    assert t.degree == 2 and t.op in (ADD, SUB, MUL)
    return Node(ADD if t.op == SUB else t.op, abs_tree(t.l), abs_tree(t.r))


def check_grad_out(val, grad, P, worst):
    """Float64: the tolerances of test_many_constants_and_deep_trees. Float32: a + - * tree of N nodes
    rounds each term of ŷ or ∂ŷ/∂c at most twice per node it passes through (the product rule's
    multiply and add), so either evaluation in T is within 2·N·u·M of the exact value, M the sum of
    the terms' absolute values (abs_tree, evaluated in float64) and u = eps(T)/2; two evaluations
    differ by at most 4·N·u·M <= 4·N·eps(T)·M, whatever the order or fusing of the operations."""
    co = P.flat.const_off
    for t in range(P.flat.ntrees):
        ref_v, ref_g = P.yhat[t].astype(np.float64), P.grads[t]
        if P.T == np.float64:
            np.testing.assert_allclose(val[t], ref_v, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(grad[co[t]:co[t + 1]], ref_g, rtol=1e-10, atol=1e-10)
            worst.add("values f64", np.abs(val[t] - ref_v), 1e-12 + 1e-12 * np.abs(ref_v))
            worst.add("gradients f64", np.abs(grad[co[t]:co[t + 1]] - ref_g), 1e-10 + 1e-10 * np.abs(ref_g))
            continue
        flat = srhip.flatten([abs_tree(P.trees[t])], opts(), dtype=np.float64)
        k, ar, _ = flat.tree(0)
        c = np.abs(P.flat.tree(t)[2].astype(np.float64))
        mv, mg, okm = oracle.eval_grad_consts(k, ar, c, np.abs(P.X.astype(np.float64)), len(c))
        assert okm
        scale = 4 * len(k) * float(np.finfo(P.T).eps)
        ev = np.abs(val[t].astype(np.float64) - ref_v)
        eg = np.abs(grad[co[t]:co[t + 1]].astype(np.float64) - ref_g)
        assert np.all(ev <= scale * mv), (P.name, t, float(np.max(ev / (scale * mv))))
        assert np.all(eg <= scale * mg), (P.name, t, float(np.max(eg / (scale * mg))))
        worst.add("values f32", ev, scale * mv)
        worst.add("gradients f32", eg, scale * mg)


@pytest.mark.parametrize("T", DTYPES, ids=lambda T: np.dtype(T).name)
@pytest.mark.parametrize("name", ["constants", "grad-deep"])
def test_per_row_gradients(gpu_ctx, name, T):
    """grad_kernel GRAD_OUT (eval_grad_tree_array): ŷ and ∂ŷ/∂c per row against the oracle's in T,
    for trees of 1 to 9 constants in the G = 1, 2, 4 passes and for the deep pass."""
    ctx = gpu_ctx
    ns = row_counts(grad_tiles(T, name))
    prog = srhip.Program(ctx, problem(name, T, ns[0]).flat, T)
    worst = Worst()
    for n in ns:
        P = problem(name, T, n)
        val, grad, ok = prog.eval_grad_tree_array(srhip.DeviceDataset(ctx, P.X, P.y))
        assert ctx.last_tree_code() == 0
        assert np.array_equal(ok, P.ok) and int(P.ok.sum()) == P.flat.ntrees
        check_grad_out(val, grad, P, worst)
    info = assert_grad_cell(prog, name)
    print(worst.line(f"{name} {np.dtype(T).name} per-row gradients n={ns} {info}"))


@pytest.mark.parametrize("name,T", CELLS)
def test_failures_across_row_groups(gpu_ctx, name, T):
    """Two row groups (n = 8192 + T0 + 1) and four trees that overflow T on one row only: x1·c and a
    tree of the family plus x1·c in row n - 1 (the last valid row of the second row group's lone
    partial tile), the same with x2 in row 0. Every loss: did_succeed as the oracle's, NaN sums for
    the failed trees (and NaN for every constant's gradient), every other tree's sum and gradient
    within its bound. Then a program of the succeeding trees alone on the same context and dataset:
    no stale failure flag may reach it."""
    ctx = gpu_ctx
    P = problem(name, T, big_n(T, name), planted=True)
    nt, nfam = P.flat.ntrees, P.nfam
    assert nt == nfam + 4 and P.ok[:nfam].all() and not P.ok[nfam:].any()  # the oracle's success count
    prog = srhip.Program(ctx, P.flat, T)
    assert prog.pass_info()["tree_code"] == 0
    worst = Worst()
    for weighted in (False, True):
        for loss in LOSS_CELLS:
            what = f"{name} {np.dtype(T).name} failing batch {lname(loss)} weighted={weighted}"
            s, wsum, ok = prog.eval_loss(dataset(ctx, P, loss, weighted), loss.kind, loss.params)
            assert ctx.last_tree_code() == 0
            check_loss_sums(s, ok, wsum, P, loss, weighted, worst, "loss", what)
        for loss in GRAD_CELLS:
            what = f"{name} {np.dtype(T).name} failing batch grad {lname(loss)} weighted={weighted}"
            sg, g, wsum, okg = prog.eval_loss_grad(dataset(ctx, P, loss, weighted), loss.kind, loss.params)
            assert ctx.last_tree_code() == 0
            check_loss_sums(sg, okg, wsum, P, loss, weighted, worst, "grad-call loss", what)
            check_loss_grads(g, P, loss, weighted, worst, what)
    # the succeeding trees alone, same context, same datasets
    Q = SimpleNamespace(**vars(P))
    Q.flat = P.flat.take(np.arange(nfam))
    Q.trees, Q.yhat, Q.ok = P.trees[:nfam], P.yhat[:nfam], P.ok[:nfam]
    prog2 = srhip.Program(ctx, Q.flat, T)
    assert_eval_cell(prog2, name, nfam)
    for weighted in (False, True):
        for loss in (L2, HUBER, srhip.L1HingeLoss(), srhip.ExpLoss()):
            what = f"{name} {np.dtype(T).name} after failures {lname(loss)} weighted={weighted}"
            ds = dataset(ctx, Q, loss, weighted)
            s, wsum, ok = prog2.eval_loss(ds, loss.kind, loss.params)
            assert np.asarray(ok).all(), what
            check_loss_sums(s, ok, wsum, Q, loss, weighted, worst, "loss after failures", what)
        for loss in (L2, srhip.L1HingeLoss()):
            what = f"{name} {np.dtype(T).name} after failures grad {lname(loss)} weighted={weighted}"
            sg, g, wsum, okg = prog2.eval_loss_grad(dataset(ctx, Q, loss, weighted), loss.kind, loss.params)
            assert np.asarray(okg).all(), what
            check_loss_sums(sg, okg, wsum, Q, loss, weighted, worst, "loss after failures", what)
            check_loss_grads(g, Q, loss, weighted, worst, what)
    assert_grad_cell(prog2, name)
    print(worst.line(f"{name} {np.dtype(T).name} n={P.n}, 4 failing trees"))


SCHEDULES = [dict(SRHIP_INTERP_DYN="0"), dict(SRHIP_INTERP_DYN="0", SRHIP_ROT="1"), dict()]


@pytest.mark.parametrize("T", DTYPES, ids=lambda T: np.dtype(T).name)
@pytest.mark.parametrize("name", ["shallow-full", "deep-eval"])
def test_schedules_give_the_same_bits(gpu_ctx, name, T):
    """The static deal of trees to waves (SRHIP_INTERP_DYN=0), the same with the row-group rotation
    (SRHIP_ROT=1) and the default (the LDS counter) — all read per launch — give the same sums,
    gradients and did_succeed bit for bit, on two row groups, with the failing trees in the batch
    (the skip path), for a generic and a margin epilogue."""
    ctx = gpu_ctx
    P = problem(name, T, big_n(T, name), planted=True)
    prog = srhip.Program(ctx, P.flat, T)
    for weighted in (False, True):
        for loss in (HUBER, srhip.L1HingeLoss()):
            ds = dataset(ctx, P, loss, weighted)
            res = []
            for sched in SCHEDULES:
                with env(**sched):
                    s, wsum, ok = prog.eval_loss(ds, loss.kind, loss.params)
                    sg, g, wsg, okg = prog.eval_loss_grad(ds, loss.kind, loss.params)
                res.append([np.array(v, copy=True) for v in (s, ok, sg, g, okg)] + [wsum, wsg])
            assert np.array_equal(res[0][1].astype(bool), P.ok) and not P.ok[P.nfam:].any()
            for other, sched in zip(res[1:], SCHEDULES[1:]):
                for a, b, what in zip(res[0], other, ("sums", "ok", "grad sums", "grads", "grad ok", "Σw", "grad Σw")):
                    assert np.array_equal(a, b, equal_nan=True), (name, lname(loss), weighted, sched, what, a, b)


def test_threaded_interpreter_gives_the_same_sums(gpu_ctx):
    """The shallow BASIC Float32 family in the threaded interpreter (SRHIP_TI=1, the default) and in
    the C++ dispatch (SRHIP_TI=0): bit-identical sums for a margin and a distance loss."""
    ctx, T, name = gpu_ctx, np.float32, "shallow-basic"
    ns = row_counts([eval_tile(T, False)])
    prog = srhip.Program(ctx, problem(name, T, ns[0]).flat, T)
    assert_eval_cell(prog, name, len(family(name)[0]))
    for n in ns:
        P = problem(name, T, n)
        for weighted in (False, True):
            for loss in (srhip.L1HingeLoss(), HUBER):
                ds = dataset(ctx, P, loss, weighted)
                res = []
                for ti in ("1", "0"):
                    with env(SRHIP_TI=ti):
                        s, wsum, ok = prog.eval_loss(ds, loss.kind, loss.params)
                    res.append((np.array(s, copy=True), np.array(ok, copy=True), wsum))
                assert res[0][1].all() and np.array_equal(res[0][1], res[1][1])
                assert np.array_equal(res[0][0], res[1][0]) and res[0][2] == res[1][2], (lname(loss), n, weighted)
