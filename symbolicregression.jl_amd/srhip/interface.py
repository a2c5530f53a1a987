"""The reference's scoring surface, evaluated on the MI355X engine.

Single-tree functions keep the reference signatures
  eval_tree_array(tree, X, options)        src/InterfaceDynamicExpressions.jl:50-52
  eval_loss(tree, dataset, options)        src/LossFunctions.jl:60-67
  score_func(dataset, tree, options)       src/LossFunctions.jl:86-92
  score_func_batch(dataset, tree, options) src/LossFunctions.jl:95-115
  update_baseline_loss_(dataset, options)  src/LossFunctions.jl:122-126
  loss_to_score(loss, baseline, tree, options)  src/LossFunctions.jl:70-83
  compute_complexity(tree, options)        src/Complexity.jl:13-40
and each has a batched form over a list of trees (one device launch), which
is what the search's callers are meant to use.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import constants as K
from .dataset import Dataset, DerivativeDataset, GroupDataset, MultiDataset
from .engine import DeviceDataset, Program, get_context
from .node import Node, count_nodes, flatten
from .options import Options

TreeOrTrees = Union[Node, Sequence[Node]]


def _as_list(trees: TreeOrTrees) -> Tuple[List[Node], bool]:
    if isinstance(trees, Node):
        return [trees], True
    return list(trees), False


def compile_trees(trees: Sequence[Node], options: Options, dtype, device: Optional[int] = None,
                  wide_tree_code: bool = False) -> Program:
    """Flatten + compile + upload a batch of trees (srhip_program_create; wide_tree_code:
    SRHIP_PROGRAM_WIDE_TREE_CODE, see Program)."""
    ctx = get_context(device)
    return Program(ctx, flatten(trees, options, dtype=dtype), dtype, wide_tree_code=wide_tree_code)


# ---- eval_tree_array ----------------------------------------------------------------
def eval_tree_array(tree: TreeOrTrees, X: np.ndarray, options: Options, device: Optional[int] = None):
    """(output, did_succeed). X is (nfeatures, n). For a list of trees the
    outputs are (ntrees, n) and did_succeed is a bool array. On failure the
    output rows are unspecified (the reference returns an undef array)."""
    trees, single = _as_list(tree)
    X = np.asarray(X)
    T = X.dtype if X.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    ctx = get_context(device)
    ds = DeviceDataset(ctx, X.astype(T, copy=False), np.zeros(X.shape[1], dtype=T))
    prog = Program(ctx, flatten(trees, options, dtype=T), T)
    out, ok = prog.eval_tree_array(ds)
    if single:
        return out[0], bool(ok[0])
    return out, ok


def _seed_features(tree: Node, plus: int, direction: Optional[int]):
    """Copy of `tree` where every feature leaf x_f (only f == direction, when
    given) becomes (x_f + c) with a new constant c = -0.0. x + (-0.0) == x for
    every x (including ±0, ±Inf, NaN), so values and did_succeed are those of
    the original tree, and ∂ŷ/∂x_f = Σ over the seeds of x_f of ∂ŷ/∂c.
    Returns the copy and, per constant in get_constants order, the feature it
    seeds (0 for the tree's own constants)."""
    def rec(t: Node) -> Node:
        if t.degree == 0:
            if t.constant or (direction is not None and t.feature != direction):
                return t.copy()
            return Node(plus, Node(feature=t.feature), Node(val=-0.0))
        if t.degree == 1:
            return Node(t.op, rec(t.l))
        return Node(t.op, rec(t.l), rec(t.r))

    aug = rec(tree)
    seeds: List[int] = []
    _mark(aug, tree, seeds)
    return aug, seeds


def _mark(aug: Node, orig: Node, seeds: List[int]) -> None:
    """Walk `aug` and the original tree together in post-order and list, per
    constant of `aug`, the feature it seeds (0 = an original constant)."""
    if orig.degree == 0:
        if orig.constant:
            seeds.append(0)
        elif aug.degree == 2:  # seeded feature leaf: (x_f + c)
            seeds.append(orig.feature)
        return
    _mark(aug.l, orig.l, seeds)
    if orig.degree == 2:
        _mark(aug.r, orig.r, seeds)


def _feature_grads(trees: List[Node], X: np.ndarray, options: Options, direction: Optional[int],
                   device: Optional[int]):
    """(ŷ (ntrees, n), per tree ∂ŷ/∂x (nfeat, n) or, with direction, (n,), ok)."""
    T = X.dtype if X.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    X = X.astype(T, copy=False)
    nfeat, n = X.shape
    if direction is not None and not 1 <= direction <= nfeat:
        raise ValueError("direction must be a 1-based feature index")
    binops = tuple(options.binary_operators)
    if "+" in binops:
        o, plus = options, binops.index("+") + 1
    else:  # same operator indices, "+" appended for the seeds
        o = Options(binary_operators=binops + ("+",), unary_operators=options.unary_operators)
        plus = len(binops) + 1
    augs, seeds = zip(*[_seed_features(t, plus, direction) for t in trees]) if trees else ((), ())
    ctx = get_context(device)
    ds = DeviceDataset(ctx, X, np.zeros(n, dtype=T))
    prog = Program(ctx, flatten(list(augs), o, dtype=T), T)
    val, grad, ok = prog.eval_grad_tree_array(ds)
    co = prog.flat.const_off
    out = []
    for t, sd in enumerate(seeds):
        g = grad[co[t]:co[t + 1]]
        sd = np.asarray(sd, dtype=np.int64)
        if direction is not None:
            d = g[sd == direction].sum(axis=0, dtype=T) if (sd == direction).any() else np.zeros(n, dtype=T)
            out.append(d.astype(T))
        else:
            G = np.zeros((nfeat, n), dtype=T)
            for f in np.unique(sd[sd > 0]):
                G[f - 1] = g[sd == f].sum(axis=0, dtype=T)
            out.append(G)
    return val, out, ok


def eval_diff_tree_array(tree: TreeOrTrees, X: np.ndarray, options: Options, direction: int,
                         device: Optional[int] = None):
    """eval_diff_tree_array(tree, X, options, direction)
    (src/InterfaceDynamicExpressions.jl:55-80): (output, ∂output/∂x_direction,
    complete), forward mode on the engine (seeded-feature tangents)."""
    trees, single = _as_list(tree)
    val, d, ok = _feature_grads(trees, np.asarray(X), options, int(direction), device)
    if single:
        return val[0], d[0], bool(ok[0])
    return val, d, ok


def eval_grad_tree_array(tree: TreeOrTrees, X: np.ndarray, options: Options, variable: bool = False,
                         device: Optional[int] = None):
    """eval_grad_tree_array(tree, X, options; variable=false)
    (src/InterfaceDynamicExpressions.jl:83-107): (output, gradient, complete)
    with gradient[k, i] = ∂ŷ_i/∂c_k for the tree's constants in get_constants
    order, or with variable=true gradient[f, i] = ∂ŷ_i/∂x_f (nfeatures × n).
    For a list of trees: outputs (ntrees, n), a list of per-tree gradient
    matrices, and a bool array."""
    trees, single = _as_list(tree)
    X = np.asarray(X)
    if variable:
        val, grads, ok = _feature_grads(trees, X, options, None, device)
        if single:
            return val[0], grads[0], bool(ok[0])
        return val, grads, ok
    T = X.dtype if X.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    ctx = get_context(device)
    ds = DeviceDataset(ctx, X.astype(T, copy=False), np.zeros(X.shape[1], dtype=T))
    prog = Program(ctx, flatten(trees, options, dtype=T), T)
    val, grad, ok = prog.eval_grad_tree_array(ds)
    co = prog.flat.const_off
    grads = [grad[co[t]:co[t + 1]] for t in range(len(trees))]
    if single:
        return val[0], grads[0], bool(ok[0])
    return val, grads, ok


# ---- derivative objectives: losses on ŷ and on ∂ŷ/∂x ----------------------------------
def _host_loss(loss, pred: np.ndarray, target: np.ndarray) -> np.ndarray:
    """The distance losses of srhip.h per row on the host, in float64
    (LossFunctions.jl's definitions on the residual r = prediction - target)."""
    name = K.LOSSES[loss.kind] if 0 <= loss.kind < len(K.LOSSES) else None
    if name is None or loss.kind >= K.MARGIN_LOSS_BEGIN:
        raise ValueError("a derivative objective takes a distance loss (L2DistLoss, L1DistLoss, HuberLoss, ...)")
    r = np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    ar = np.abs(r)
    p = float(loss.param)
    with np.errstate(all="ignore"):
        if name == "L2":
            return r * r
        if name == "L1":
            return ar
        if name in ("LP", "LPINT"):
            return ar ** p
        if name == "HUBER":
            return np.where(ar <= p, 0.5 * r * r, p * (ar - 0.5 * p))
        if name == "LOGCOSH":
            return ar + np.log1p(np.exp(-2.0 * ar)) - np.log(2.0)
        if name == "L1EPSINS":
            return np.maximum(ar - p, 0.0)
        if name == "L2EPSINS":
            return np.maximum(ar - p, 0.0) ** 2
        if name == "QUANTILE":
            return np.where(r >= 0.0, p * r, (p - 1.0) * r)
        if name == "PERIODIC":
            return 1.0 - np.cos(r * (2.0 * np.pi / p))
        return ar + 2.0 * np.log1p(np.exp(-ar)) - np.log(4.0)  # LOGITDIST


class DerivativeObjective:
    """A `loss_function` that scores the prediction and its derivatives with
    respect to features ("a loss that takes into account derivatives",
    src/Options.jl:203-210): Σ_k coefficients[k] · mean_k, where mean_0 is the
    weighted mean of ℓ(ŷ, y) and mean_{1+j} that of ℓ(∂ŷ/∂x_d, dydx[j]) along
    d = dataset.directions[j], over a DerivativeDataset. ℓ is `elementwise_loss`
    (a distance loss; default: options.elementwise_loss). +Inf when the tree
    fails or the result is not finite.

    Called as f(tree, dataset, options) it evaluates one tree through
    eval_tree_array and eval_diff_tree_array, so it is a valid
    options.loss_function anywhere; eval_loss_batch_ok recognises it on a
    DerivativeDataset and scores the whole batch in one fused engine call
    (eval_deriv_loss_batch). `eval_tree_array` / `eval_diff_tree_array` replace the
    two evaluators of the per-tree call (tests run it on a CPU evaluator)."""

    def __init__(self, coefficients: Sequence[float], elementwise_loss=None, eval_tree_array=None,
                 eval_diff_tree_array=None):
        c = np.asarray(coefficients, dtype=np.float64)
        if c.ndim != 1 or len(c) < 2:
            raise ValueError("coefficients must hold one value per channel: y, then one per direction")
        if not np.isfinite(c).all():
            raise ValueError("coefficients must be finite")
        if elementwise_loss is not None and (not hasattr(elementwise_loss, "kind")
                                             or not 0 <= elementwise_loss.kind < K.MARGIN_LOSS_BEGIN):
            raise ValueError("a derivative objective takes a distance loss (L2DistLoss, L1DistLoss, HuberLoss, ...)")
        self.coefficients = c
        self.elementwise_loss = elementwise_loss
        self._eval = eval_tree_array
        self._diff = eval_diff_tree_array

    def loss(self, options: Options):
        loss = self.elementwise_loss if self.elementwise_loss is not None else options.elementwise_loss
        if not hasattr(loss, "kind") or not 0 <= loss.kind < K.MARGIN_LOSS_BEGIN:
            raise ValueError("a derivative objective takes a distance loss (L2DistLoss, L1DistLoss, HuberLoss, ...)")
        return loss

    def check(self, dataset) -> "DerivativeDataset":
        if not isinstance(dataset, DerivativeDataset):
            raise ValueError("a DerivativeObjective scores a DerivativeDataset")
        if len(self.coefficients) != 1 + dataset.ndir:
            raise ValueError(f"{len(self.coefficients)} coefficients for {1 + dataset.ndir} channels "
                             "(y, then one per direction)")
        return dataset

    def combine(self, means: np.ndarray, ok: np.ndarray, T) -> np.ndarray:
        """Σ_k coefficients[k] · means[:, k] in float64, cast to T; +Inf where !ok or not finite."""
        with np.errstate(all="ignore"):
            v = np.asarray(means, dtype=np.float64) @ self.coefficients
            out = v.astype(T)
        out[~(np.asarray(ok, dtype=bool) & np.isfinite(v))] = T(np.inf)
        return out

    def __call__(self, tree: Node, dataset, options: Options):
        ds = self.check(dataset)
        loss = self.loss(options)
        ev = self._eval if self._eval is not None else eval_tree_array
        df = self._diff if self._diff is not None else eval_diff_tree_array
        T = ds.T
        W = ds.multi.weights
        val, ok = ev(tree, ds.X, options)
        if not ok:
            return T(np.inf)
        chans = [(val, ds.y)]
        for j, d in enumerate(ds.directions):
            _, g, okd = df(tree, ds.X, options, d)
            if not okd:
                return T(np.inf)
            chans.append((g, ds.dydx[j]))
        means = np.empty(len(chans), dtype=np.float64)
        for k, (pred, tgt) in enumerate(chans):
            l = _host_loss(loss, pred, tgt)
            with np.errstate(all="ignore"):
                if W is None:
                    means[k] = l.sum() / ds.n
                else:
                    w = np.asarray(W[k], dtype=np.float64)
                    means[k] = (w * l).sum() / w.sum()
        return self.combine(means[None, :], np.ones(1, dtype=bool), T)[0]


def eval_deriv_loss_batch(trees: Sequence[Node], dataset: DerivativeDataset, options: Options,
                          device: Optional[int] = None, elementwise_loss=None):
    """The channel means of a derivative objective for many trees in one fused
    engine call (srhip_eval_loss_deriv): (means [ntrees, 1 + ndir] in float64 —
    column 0 the weighted mean of ℓ(ŷ, y), column 1 + j that of
    ℓ(∂ŷ/∂x_d, dydx[j]) along d = dataset.directions[j] — and did_succeed per
    tree). A failed tree's row is NaN. ℓ is elementwise_loss (default:
    options.elementwise_loss), a distance loss."""
    if not isinstance(dataset, DerivativeDataset):
        raise ValueError("eval_deriv_loss_batch scores a DerivativeDataset")
    loss = elementwise_loss if elementwise_loss is not None else options.elementwise_loss
    if not hasattr(loss, "kind") or not 0 <= loss.kind < K.MARGIN_LOSS_BEGIN:
        raise ValueError("a derivative objective takes a distance loss (L2DistLoss, L1DistLoss, HuberLoss, ...)")
    trees = list(trees)
    T = dataset.T
    dev = dataset.multi.device(device)
    prog = Program(dev.ctx, flatten(trees, options, dtype=T), T, interpreted=True)
    sums, wsum, ok = prog.eval_loss_deriv(dev, loss.kind, [d - 1 for d in dataset.directions], loss.params)
    with np.errstate(invalid="ignore", divide="ignore"):
        means = sums / wsum[None, :]
    return means, ok


def eval_deriv_loss_grad_batch(trees: Sequence[Node], dataset: DerivativeDataset, options: Options,
                               device: Optional[int] = None):
    """The objective values of options.loss_function (a DerivativeObjective) and their
    gradients with respect to the trees' constants, in one fused engine call
    (srhip_eval_loss_grad_deriv): (values [ntrees] in float64, +Inf where the tree
    fails or the value is not finite; ∂objective/∂c [total constants, in the trees'
    order], NaN for a failed tree; did_succeed per tree)."""
    obj = options.loss_function
    if not isinstance(obj, DerivativeObjective):
        raise ValueError("eval_deriv_loss_grad_batch needs a DerivativeObjective as options.loss_function")
    ds = obj.check(dataset)
    loss = obj.loss(options)
    trees = list(trees)
    T = ds.T
    dev = ds.multi.device(device)
    flat = flatten(trees, options, dtype=T)
    prog = Program(dev.ctx, flat, T, interpreted=True)
    sums, grads, wsum, ok = prog.eval_loss_grad_deriv(dev, loss.kind, [d - 1 for d in ds.directions], loss.params)
    with np.errstate(all="ignore"):
        v = np.zeros(len(trees))
        g = np.zeros(grads.shape[0])
        for c in range(1 + ds.ndir):  # channel order, as srhip_optimize_constants_deriv
            v = v + obj.coefficients[c] * sums[:, c] / wsum[c]
            g = g + obj.coefficients[c] * grads[:, c] / wsum[c]
    v[~(ok & np.isfinite(v))] = np.inf
    g[np.repeat(~ok, np.diff(flat.const_off))] = np.nan
    return v, g, ok


def _eval_loss_grad_targets(trees, dataset, options: Options, device, row_idx, targets, fused):
    """eval_loss_grad_batch on a MultiDataset: one fused call (srhip_eval_loss_grad_targets,
    with row_idx srhip_eval_loss_grad_rowsets_targets), or the trees regrouped by target and
    each group on its view."""
    tg = _check_targets(trees, dataset, targets)
    R = None if row_idx is None else _check_row_sets(row_idx, len(trees))
    loss = options.elementwise_loss
    T = dataset.T
    if fused is None:
        fused = len(trees) <= FUSED_GRAD_TARGETS_MAX_TREES
    if not fused or loss.kind >= K.EXPR_LOSS_BEGIN:  # expression losses: views
        losses = np.zeros(len(trees), dtype=T)
        ok = np.zeros(len(trees), dtype=bool)
        g = [None] * len(trees)
        for k in np.unique(tg):
            idx = np.flatnonzero(tg == k)
            lv, gv, kv = eval_loss_grad_batch([trees[t] for t in idx], dataset.target(int(k)), options, device,
                                              None if R is None else R[idx])
            losses[idx] = lv
            ok[idx] = kv
            for j, t in enumerate(idx):
                g[t] = gv[j]
        return losses, g, ok
    dev = dataset.device(device)
    prog = Program(dev.ctx, flatten(trees, options, dtype=T), T, interpreted=True)
    if R is None:
        sums, grads, wsum, ok = prog.eval_loss_grad_targets(dev, loss.kind, tg, loss.params)
        wsums = wsum[tg]
    else:
        sums, grads, wsums, ok = prog.eval_loss_grad_rowsets_targets(dev, loss.kind, tg, R, loss.params)
    with np.errstate(invalid="ignore", divide="ignore"):
        losses = (sums / wsums).astype(T)
        co = prog.flat.const_off
        g = [grads[co[t]:co[t + 1]] / wsums[t] for t in range(len(trees))]
    losses[~ok] = T(np.inf)
    return losses, g, ok


def eval_loss_grad_batch(trees: Sequence[Node], dataset: Dataset, options: Options,
                         device: Optional[int] = None, row_idx: Optional[np.ndarray] = None,
                         targets: Optional[Sequence[int]] = None, fused: Optional[bool] = None):
    """Batched loss + constant gradients for ConstantOptimization
    (src/ConstantOptimization.jl:12-65): per tree (loss in T, ∂loss/∂c as a
    float64 vector in get_constants order, did_succeed). A GroupDataset runs
    over its device group (`device` is then unused). row_idx, an
    (ntrees, batch_size) integer array: tree t on its own row sample row_idx[t]
    (srhip_eval_loss_grad_rowsets), loss and gradient divided by that sample's
    Σw; not on a GroupDataset. A MultiDataset takes targets (one target index
    per tree): tree t against target targets[t], each loss and gradient divided
    by its own target's Σw, in one fused call up to
    FUSED_GRAD_TARGETS_MAX_TREES trees and on per-target views beyond; `fused`
    forces either."""
    if isinstance(dataset, MultiDataset):
        return _eval_loss_grad_targets(list(trees), dataset, options, device, row_idx, targets, fused)
    if targets is not None:
        raise ValueError("targets= needs a MultiDataset")
    loss = options.elementwise_loss
    if row_idx is not None:
        if isinstance(dataset, GroupDataset):
            raise ValueError("row_idx is not supported on a GroupDataset")
        R = _check_row_sets(row_idx, len(trees))
        dev = dataset.device(device)
        T = dataset.T
        prog = Program(dev.ctx, flatten(trees, options, dtype=T), T, interpreted=True)
        sums, grads, wsums, ok = prog.eval_loss_grad_rowsets(dev, loss.kind, R, loss.params)
        with np.errstate(invalid="ignore", divide="ignore"):
            losses = (sums / wsums).astype(T)
            co = prog.flat.const_off
            g = [grads[co[t]:co[t + 1]] / wsums[t] for t in range(len(trees))]
        losses[~ok] = T(np.inf)
        return losses, g, ok
    if isinstance(dataset, GroupDataset):
        prog = dataset.group.program(flatten(trees, options, dtype=dataset.T), dataset.T)
        sums, grads, wsum, ok = prog.eval_loss_grad(dataset, loss.kind, loss.params)
        prog.close()
    else:
        dev = dataset.device(device)
        prog = compile_trees(trees, options, dataset.T, dev.ctx.device)
        sums, grads, wsum, ok = prog.eval_loss_grad(dev, loss.kind, loss.params)
    T = dataset.T
    with np.errstate(invalid="ignore", divide="ignore"):
        losses = (sums / wsum).astype(T)
    losses[~ok] = T(np.inf)
    co = prog.flat.const_off
    g = [grads[co[t]:co[t + 1]] / wsum for t in range(len(trees))]
    return losses, g, ok


def _check_row_sets(row_idx, ntrees: int) -> np.ndarray:
    """An (ntrees, batch_size) integer array of row samples, one per tree."""
    R = np.asarray(row_idx)
    if R.ndim != 2 or R.shape[0] != ntrees:
        raise ValueError(f"row_idx must be (ntrees, batch_size) = ({ntrees}, batch_size), not {R.shape}")
    if R.size and not np.issubdtype(R.dtype, np.integer):
        raise ValueError("row_idx must hold integers")
    return np.ascontiguousarray(R, dtype=np.int64)


# ---- losses -------------------------------------------------------------------------
def eval_loss_batch(trees: Sequence[Node], dataset: Dataset, options: Options,
                    row_idx: Optional[np.ndarray] = None, device: Optional[int] = None,
                    program: Optional[Program] = None) -> np.ndarray:
    """eval_loss for many trees in one launch: the reference's `_eval_loss`
    value in T per tree (T(Inf) where the evaluation fails)."""
    return eval_loss_batch_ok(trees, dataset, options, row_idx, device, program)[0]


# Trees per call up to which a MultiDataset's candidates are scored by the fused
# call; larger batches go to per-target views (regroup, score, scatter back).
# The fused call always runs in the interpreter and a view call runs tree code from
# 256 shallow trees on (api.cpp jit_wanted, SRHIP_JIT), so the expected switch was
# 256. Measured (tools/bench_targets.py, profiles/targets_timing.json; Float32, L2,
# 5 features, K = 4; one step = a program built, scored and destroyed per call, as
# these functions do): 4 x 66 trees on 100k rows: fused 0.37 ms, four view calls
# 0.58 ms; 4 x 1024 trees on 1M rows: fused 8.8 ms (kernels 7.4), four view calls
# 52-58 ms (kernels 17.9, the rest building and loading tree code for one use). No
# crossover up to 4096 trees, the largest batch measured: the fused call is used up
# to there and the views beyond it. A caller that keeps its programs (srhip.Program on
# mds.target(k).device()) pays for the tree code once and is not covered by this.
FUSED_TARGETS_MAX_TREES = 4096

# Trees per call up to which a MultiDataset's gradients and constant optimisation
# run fused (srhip_eval_loss_grad_targets, srhip_optimize_constants_targets); larger
# batches are regrouped by target and run on the views, whose gradient passes are
# reverse-mode tree code from 256 candidates per program on. Set from the measured
# table (tools/bench_grad_targets.py, profiles/grad_targets_timing.json, DESIGN.md
# §3.17): the largest measured batch at which all three fused medians lie below the
# views' three. Float32, L2, 5 features, K = 4, 8 BFGS iterations, 1 + 2 starts:
# 4 x 33 trees on 100k rows: fused 73 ms, four view runs 145-148 ms; 4 x 256 trees:
# fused 273-275 ms, views 362-363 ms. The ratio falls from 2.0 to 1.3 over that range;
# nothing above 1024 trees was measured, so the views take over there (fused=True
# forces the fused path).
FUSED_GRAD_TARGETS_MAX_TREES = 1024


def _check_targets(trees, dataset: MultiDataset, targets) -> np.ndarray:
    if targets is None:
        if dataset.ntargets > 1:
            raise ValueError("a MultiDataset with several targets needs targets= (one target index per tree), "
                             "or score dataset.target(k)")
        targets = np.zeros(len(trees), dtype=np.int32)
    tg = np.asarray(targets)
    if tg.shape != (len(trees),):
        raise ValueError("targets must have one entry per tree")
    if len(tg) and (tg.min() < 0 or tg.max() >= dataset.ntargets):
        raise ValueError("target index out of range")
    return tg.astype(np.int32)


def _scatter_by_target(trees, dataset: MultiDataset, tg: np.ndarray, fn):
    """Regroup the trees by target, score each group with fn(subtrees, dataset.target(k), positions),
    scatter the (losses, ok) back."""
    losses = np.zeros(len(trees), dtype=dataset.T)
    ok = np.zeros(len(trees), dtype=bool)
    for k in np.unique(tg):
        idx = np.flatnonzero(tg == k)
        lv, kv = fn([trees[t] for t in idx], dataset.target(int(k)), idx)
        losses[idx] = lv
        ok[idx] = kv
    return losses, ok


def _eval_loss_targets(trees, dataset: MultiDataset, options: Options, row_idx, device, targets, fused):
    tg = _check_targets(trees, dataset, targets)
    if options.loss_function is not None:
        return _scatter_by_target(trees, dataset, tg,
                                  lambda sub, ds, idx: eval_loss_batch_ok(sub, ds, options, row_idx, device))
    loss = options.elementwise_loss
    if fused is None:
        fused = len(trees) <= FUSED_TARGETS_MAX_TREES
    # the fused call covers all rows and the table losses; everything else goes through views
    if not fused or row_idx is not None or loss.kind >= K.EXPR_LOSS_BEGIN:
        return _scatter_by_target(trees, dataset, tg,
                                  lambda sub, ds, idx: eval_loss_batch_ok(sub, ds, options, row_idx, device))
    T = dataset.T
    dev = dataset.device(device)
    prog = Program(dev.ctx, flatten(trees, options, dtype=T), T, interpreted=True)
    sums, wsum, ok = prog.eval_loss_targets(dev, loss.kind, tg, loss.params)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (sums / wsum[tg]).astype(T)
    out[~ok] = T(np.inf)
    return out, ok


def eval_loss_batch_ok(trees: Sequence[Node], dataset: Dataset, options: Options,
                       row_idx: Optional[np.ndarray] = None, device: Optional[int] = None,
                       program: Optional[Program] = None, targets: Optional[Sequence[int]] = None,
                       fused: Optional[bool] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(losses in T, did_succeed per tree). A GroupDataset runs over its
    device group (all rows: no row_idx there; `program`, if given, a
    GroupProgram of that group; `device` unused). A MultiDataset takes
    targets (one target index per tree) and scores tree t against target
    targets[t]: in one fused launch up to FUSED_TARGETS_MAX_TREES trees, on
    per-target views (regroup, score, scatter back) beyond; `fused` forces
    either."""
    if isinstance(dataset, MultiDataset):
        if program is not None:
            raise ValueError("program= is not supported with a MultiDataset")
        return _eval_loss_targets(list(trees), dataset, options, row_idx, device, targets, fused)
    if targets is not None:
        raise ValueError("targets= needs a MultiDataset")
    if isinstance(options.loss_function, DerivativeObjective) and isinstance(dataset, DerivativeDataset):
        # the fused call: every channel of every tree in one pass (all rows, the program built here)
        if row_idx is not None or program is not None:
            raise ValueError("a DerivativeObjective scores all rows of its DerivativeDataset; row_idx= and program= "
                             "are not supported with it")
        f = options.loss_function
        f.check(dataset)
        means, ok = eval_deriv_loss_batch(trees, dataset, options, device, f.loss(options))
        out = f.combine(means, ok, dataset.T)
        return out, ok & np.isfinite(out)
    if options.loss_function is not None:
        f = options.loss_function
        vals = np.asarray([f(t, dataset, options) for t in trees], dtype=dataset.T)
        return vals, np.isfinite(vals)
    loss = options.elementwise_loss
    if isinstance(dataset, GroupDataset):
        if row_idx is not None:
            raise ValueError("row_idx is not supported on a GroupDataset")
        prog = program if program is not None else dataset.group.program(
            flatten(trees, options, dtype=dataset.T), dataset.T)
        sums, wsum, ok = prog.eval_loss(dataset, loss.kind, loss.params)
        if program is None:
            prog.close()
    else:
        dev = dataset.device(device)
        prog = program if program is not None else compile_trees(trees, options, dataset.T, dev.ctx.device)
        sums, wsum, ok = prog.eval_loss(dev, loss.kind, loss.params, row_idx)
    T = dataset.T
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (sums / wsum).astype(T)
    out[~ok] = T(np.inf)
    return out, ok


def eval_loss_batch_rowsets(trees: Sequence[Node], dataset: Dataset, options: Options,
                            rows: Sequence[np.ndarray], device: Optional[int] = None,
                            targets: Optional[Sequence[int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """score_func_batch's evaluation for many trees, tree t on its OWN row
    sample rows[t] (with replacement, LossFunctions.jl:95-115; the reference
    draws one sample per call, :98): (losses in T, did_succeed). One engine
    launch for all trees (srhip_eval_loss_rowsets) when the samples have one
    length (the reference's batch_size); one per distinct length otherwise.
    score_func_batch uses options.elementwise_loss even when loss_function is
    set (:101-111), and so does this. A MultiDataset takes targets (one target
    index per tree): tree t's sample is scored against target targets[t], still
    in one launch (srhip_eval_loss_rowsets_targets)."""
    T = dataset.T
    n = len(trees)
    losses = np.zeros(n, dtype=T)
    ok = np.zeros(n, dtype=bool)
    multi = isinstance(dataset, MultiDataset)
    if multi:
        tg = _check_targets(trees, dataset, targets)
    elif targets is not None:
        raise ValueError("targets= needs a MultiDataset")
    if n == 0:
        return losses, ok
    rows = [np.asarray(r, dtype=np.int64) for r in rows]
    if len(rows) != n:
        raise ValueError("one row sample per tree")
    loss = options.elementwise_loss
    if multi and loss.kind >= K.EXPR_LOSS_BEGIN:  # expression losses: views
        return _scatter_by_target(list(trees), dataset, tg,
                                  lambda sub, ds, idx: eval_loss_batch_rowsets(sub, ds, options,
                                                                               [rows[t] for t in idx], device))
    dev = dataset.device(device)
    by_len = {}
    for t, r in enumerate(rows):
        by_len.setdefault(len(r), []).append(t)
    for bs, idx in by_len.items():
        sub = [trees[t] for t in idx]
        prog = Program(dev.ctx, flatten(sub, options, dtype=T), T, interpreted=True)
        R = np.stack([rows[t] for t in idx]) if bs else np.zeros((len(idx), 0), dtype=np.int64)
        if multi:
            sums, wsum, k = prog.eval_loss_rowsets_targets(dev, loss.kind, tg[idx], R, loss.params)
        else:
            sums, wsum, k = prog.eval_loss_rowsets(dev, loss.kind, R, loss.params)
        with np.errstate(invalid="ignore", divide="ignore"):
            lv = (sums / wsum).astype(T)
        lv[~k] = T(np.inf)
        losses[idx] = lv
        ok[idx] = k
    return losses, ok


def eval_loss(tree: Node, dataset: Dataset, options: Options) -> float:
    return eval_loss_batch([tree], dataset, options)[0]


def compute_complexity(tree: Node, options: Options) -> int:
    if not options.complexity_use:
        return count_nodes(tree)

    def rec(t: Node) -> float:
        if t.degree == 0:
            return options.constant_complexity if t.constant else options.variable_complexity
        if t.degree == 1:
            return options.unaop_complexities[t.op - 1] + rec(t.l)
        return options.binop_complexities[t.op - 1] + rec(t.l) + rec(t.r)

    return int(round(rec(tree)))


def loss_to_score(loss, baseline, tree: Node, options: Options):
    """LossFunctions.jl:69-82 in T; the parsimony term is Int × Float32
    (options.parsimony is a Float32 field, Options.jl:327)."""
    T = type(loss) if isinstance(loss, np.floating) else np.float64
    normalization = T(0.01) if baseline < T(0.01) else T(baseline)
    term = np.float32(compute_complexity(tree, options)) * np.float32(options.parsimony)
    with np.errstate(all="ignore"):
        return T(T(loss / normalization) + T(term))


def score_func_batched(dataset: Dataset, trees: Sequence[Node], options: Options,
                       device: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """score_func over many trees: (scores, losses)."""
    losses = eval_loss_batch(trees, dataset, options, device=device)
    scores = np.asarray([loss_to_score(l, dataset.baseline_loss, t, options) for l, t in zip(losses, trees)],
                        dtype=dataset.T)
    return scores, losses


def score_func(dataset: Dataset, tree: Node, options: Options):
    s, l = score_func_batched(dataset, [tree], options)
    return s[0], l[0]


def score_func_batch(dataset: Dataset, tree: TreeOrTrees, options: Options,
                     rng: Optional[np.random.Generator] = None, row_idx: Optional[np.ndarray] = None):
    """Minibatch score (src/LossFunctions.jl:95-115): batch_size rows sampled
    with replacement; a failed evaluation scores (0, Inf) as in the reference."""
    trees, single = _as_list(tree)
    if row_idx is None:
        rng = rng or np.random.default_rng()
        row_idx = rng.integers(0, dataset.n, size=options.batch_size)
    losses, ok = eval_loss_batch_ok(trees, dataset, options, row_idx=row_idx)
    T = dataset.T
    scores = np.asarray(
        [loss_to_score(l, dataset.baseline_loss, t, options) if k else T(0)
         for l, t, k in zip(losses, trees, ok)],
        dtype=T,
    )
    if single:
        return scores[0], losses[0]
    return scores, losses


def update_baseline_loss_(dataset: Dataset, options: Options) -> None:
    """update_baseline_loss!: loss of the constant tree avg_y."""
    dataset.baseline_loss = eval_loss(Node(val=dataset.avg_y), dataset, options)
