"""Batched constant optimisation: the Python mirror
of `optimize_constants` (src/ConstantOptimization.jl:22-65) for a whole
population, over libsrhip's lockstep optimiser (csrc/constopt.cpp).

The reference optimises one PopMember at a time: Optim.Newton (one
constant) or Optim.BFGS — or NelderMead (:35-36) — with
LineSearches.BackTracking, `optimizer_iterations` = 8 (src/Options.jl:607-621),
from x0 and from `optimizer_nrestarts` = 2 perturbed starts x0 .* (1 + randn/2)
(:46-54); the best run is kept if Optim reports convergence, else the
constants go back to x0 (:56-63).

Here every start of every tree is a candidate and all candidates advance in
lockstep inside libsrhip (srhip_optimize_constants_batch): each phase of an
iteration is ONE launch over all of them (srhip_program_set_constants +
srhip_eval_loss_grad / srhip_eval_loss). The per-candidate algebra runs in
C++ next to the engine; this module draws the start noise (from the caller's
numpy Generator, tree by tree, restart by restart — where the reference
calls randn) and writes the results back into the trees.

`evaluator_factory` plugs any other evaluator into the same C++ driver
through srhip_optimize_constants_cb (a row-sharded dataset whose partials
are all-reduced, the oracle in tests): factory(candidates) returns an object
with loss_grad(consts) -> (f, g) and loss_only(consts) -> f. No part of the
optimiser runs in Python; tests/constopt_reference.py restates it as the
checker.
"""
from __future__ import annotations

import ctypes as C
import inspect
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np

from ._lib import CONSTOPT_EVAL_FN, ConstOptOptions, check, lib
from .dataset import Dataset, DerivativeDataset, GroupDataset, MultiDataset
from .engine import _trees_struct
from .node import Node, flatten, set_constants
from .options import Options

ALGORITHMS = {"BFGS": 0, "NelderMead": 1}  # SRHIP_OPT_*


@dataclass
class ConstOptResult:
    """Per input tree: the loss after optimisation (the reference re-scores a
    converged member, :56-60; else the loss at x0), Optim's convergence flag of
    the best start, and the number of loss evaluations (num_evals)."""

    losses: np.ndarray
    converged: np.ndarray
    num_evals: np.ndarray


def _finish(sums, wsum, ok) -> np.ndarray:
    """Loss of each candidate from engine partials (:12-19): Σw·ℓ/Σw, +Inf on failure."""
    with np.errstate(invalid="ignore", divide="ignore"):
        f = sums / wsum
    return np.where(ok & np.isfinite(f), f, np.inf)


def _grad_finish(grads, wsum, ok, const_off) -> np.ndarray:
    """∂L/∂c of each constant from engine partials, NaN for failed candidates."""
    g = grads / wsum
    g[np.repeat(~ok, np.diff(const_off))] = np.nan
    return g


def start_noise(flat, nrestarts: int, rng: np.random.Generator) -> np.ndarray:
    """The standard normal draws of the perturbed starts in the C ABI's order
    (tree by tree, restart by restart, :46-54)."""
    co = flat.const_off
    parts = []
    for i in range(flat.ntrees):
        n = int(co[i + 1] - co[i])
        for _ in range(nrestarts if n else 0):
            parts.append(rng.standard_normal(n))
    return np.concatenate(parts) if parts else np.zeros(0)


def optimize_constants_batch(dataset: Dataset, trees: Sequence[Node], options: Options,
                             rng: Optional[np.random.Generator] = None, device: Optional[int] = None,
                             evaluator_factory: Optional[Callable] = None,
                             noise: Optional[np.ndarray] = None,
                             row_idx: Optional[np.ndarray] = None,
                             targets: Optional[Sequence[int]] = None,
                             fused: Optional[bool] = None) -> ConstOptResult:
    """`optimize_constants` for many trees at once. Trees are updated in place
    (constants of the best start when it converged, else left at x0).
    `noise` (default: drawn from `rng`) is the standard normal draws of the
    perturbed starts in start_noise's order, for callers that draw them
    where the reference does (srhip.evolution: from each island's stream).
    `row_idx`, an (ntrees, batch_size) integer array: tree t is optimised on its
    own row sample row_idx[t], the same rows for all of its starts, iterations
    and the final evaluation (srhip_optimize_constants_rowsets; the losses are
    those on the samples, num_evals counts evaluations as without it). Not on a
    GroupDataset. With `evaluator_factory` the evaluator owns the rows: a factory
    whose signature accepts `members=` is given the input tree index of each
    candidate and picks their samples itself.
    A MultiDataset takes `targets` (one target index per tree): tree t is
    optimised against target targets[t], the populations of all outputs in one
    lockstep run (srhip_optimize_constants_targets) up to
    interface.FUSED_GRAD_TARGETS_MAX_TREES trees. Larger batches, expression
    losses, `loss_function` and `evaluator_factory` regroup the trees by target
    and optimise each group on dataset.target(k) with its slice of the start
    noise (a factory whose signature accepts `target=` is told k); `fused`
    forces either where both apply. The noise array is the same either way:
    start_noise's order over the trees as given."""
    if isinstance(dataset, DerivativeDataset):
        raise ValueError("a DerivativeDataset is not supported by optimize_constants_batch, which fits ŷ to one target: "
                         "optimize_constants_deriv_batch fits the constants under a DerivativeObjective, and "
                         "dataset.target(0) is the Dataset of the value alone")
    multi = isinstance(dataset, MultiDataset)
    if multi:
        from .interface import _check_targets

        tg = _check_targets(trees, dataset, targets)
    elif targets is not None:
        raise ValueError("targets= needs a MultiDataset")
    if row_idx is not None:
        from .interface import _check_row_sets

        if isinstance(dataset, GroupDataset):
            raise ValueError("row_idx is not supported on a GroupDataset")
        row_idx = _check_row_sets(row_idx, len(trees))
    algorithm = getattr(options, "optimizer_algorithm", "BFGS")
    if algorithm not in ALGORITHMS:
        raise ValueError("Optimization function not implemented.")  # :39-41
    T = np.dtype(dataset.T).type
    flat = flatten(trees, options, dtype=T)
    nrestarts = int(getattr(options, "optimizer_nrestarts", 2))
    if noise is None:
        noise = start_noise(flat, nrestarts, rng or np.random.default_rng())
    noise = np.ascontiguousarray(noise, dtype=np.float64)
    need = int(sum(nrestarts * int(flat.const_off[i + 1] - flat.const_off[i]) for i in range(flat.ntrees)))
    if noise.shape != (need,):
        raise ValueError(f"start noise has {noise.size} values, the trees' restarts need {need}")
    loss = options.elementwise_loss
    if multi:
        from . import constants as K
        from .interface import FUSED_GRAD_TARGETS_MAX_TREES

        if fused is None:
            fused = len(trees) <= FUSED_GRAD_TARGETS_MAX_TREES
        if (not fused or evaluator_factory is not None or options.loss_function is not None
                or loss.kind >= K.EXPR_LOSS_BEGIN):
            return _optimize_by_target(dataset, trees, options, device, evaluator_factory, noise, row_idx, tg,
                                       flat.const_off, nrestarts)
    par = None if loss.params is None else np.ascontiguousarray(loss.params, dtype=np.float64)
    opts = ConstOptOptions(ALGORITHMS[algorithm], int(getattr(options, "optimizer_iterations", 8)), nrestarts,
                           int(loss.kind), None if par is None else par.ctypes.data_as(C.POINTER(C.c_double)),
                           noise.ctypes.data_as(C.POINTER(C.c_double)), 0)
    consts = np.ascontiguousarray(flat.consts, dtype=T)
    tr = _trees_struct(flat, consts)
    nt = len(trees)
    out_c = np.zeros(max(consts.size, 1), dtype=T)
    out_l = np.zeros(max(nt, 1))
    out_k = np.zeros(max(nt, 1), dtype=np.uint8)
    out_n = np.zeros(max(nt, 1))
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in (out_c, out_l, out_k, out_n)]
    if multi:
        dev = dataset.device(device)
        tgc = np.ascontiguousarray(tg, dtype=np.int32)
        check(lib().srhip_optimize_constants_targets(
            dev.ctx.handle, dev.handle, C.byref(tr), C.byref(opts), tgc.ctypes.data_as(C.c_void_p),
            None if row_idx is None else row_idx.ctypes.data_as(C.c_void_p),
            0 if row_idx is None else row_idx.shape[1], *ptrs))
    elif evaluator_factory is None and isinstance(dataset, GroupDataset):
        # the rows sharded over a device group (srhip_group_optimize_constants)
        check(lib().srhip_group_optimize_constants(dataset.handle, C.byref(tr), C.byref(opts), *ptrs))
    elif evaluator_factory is None and row_idx is not None:
        dev = dataset.device(device)
        check(lib().srhip_optimize_constants_rowsets(dev.ctx.handle, dev.handle, C.byref(tr), C.byref(opts),
                                                     row_idx.ctypes.data_as(C.c_void_p), row_idx.shape[1], *ptrs))
    elif evaluator_factory is None:
        dev = dataset.device(device)
        check(lib().srhip_optimize_constants_batch(dev.ctx.handle, dev.handle, C.byref(tr), C.byref(opts), *ptrs))
    else:
        cb = _Callback(trees, evaluator_factory)
        rc = lib().srhip_optimize_constants_cb(C.byref(tr), 0 if T == np.float32 else 1, C.byref(opts),
                                               cb.fn, None, *ptrs)
        if cb.error is not None:
            raise cb.error
        check(rc)
    conv = out_k[:nt].astype(bool)
    co = flat.const_off
    for i in np.flatnonzero(conv):
        set_constants(trees[i], [T(v) for v in out_c[co[i]:co[i + 1]]])
    return ConstOptResult(out_l[:nt].copy(), conv, out_n[:nt].copy())


def optimize_constants_deriv_batch(dataset: DerivativeDataset, trees: Sequence[Node], options: Options,
                                   rng: Optional[np.random.Generator] = None, device: Optional[int] = None,
                                   evaluator_factory: Optional[Callable] = None, noise: Optional[np.ndarray] = None,
                                   row_idx: Optional[np.ndarray] = None,
                                   targets: Optional[Sequence[int]] = None) -> ConstOptResult:
    """`optimize_constants` for many trees at once on a DerivativeDataset under
    options.loss_function, a DerivativeObjective (srhip_optimize_constants_deriv): the constants
    are fitted to Σ_c coefficients[c] · mean_c over y and every derivative channel, with analytic
    gradients (∂²ŷ/∂c∂x). Trees are updated in place as optimize_constants_batch updates them;
    `rng` / `noise` as there. The losses are the objective's values in float64. All rows are
    scored on one device: `row_idx=`, `targets=` and `evaluator_factory=` are refused by name, as
    are margin and expression losses."""
    from .interface import DerivativeObjective

    obj = options.loss_function
    if not isinstance(obj, DerivativeObjective):
        raise ValueError("constant optimisation on a DerivativeDataset is not supported without a DerivativeObjective as "
                         "options.loss_function: optimise on dataset.target(0) to fit the value alone")
    obj.check(dataset)
    if row_idx is not None:
        raise ValueError("row_idx= is not supported under a derivative objective in this version (all rows are scored)")
    if targets is not None:
        raise ValueError("targets= is not supported under a derivative objective: its channels are the targets")
    if evaluator_factory is not None:
        raise ValueError("evaluator_factory= is not supported under a derivative objective in this version")
    loss = obj.loss(options)  # (a distance loss: margin and expression losses are refused there)
    algorithm = getattr(options, "optimizer_algorithm", "BFGS")
    if algorithm not in ALGORITHMS:
        raise ValueError("Optimization function not implemented.")  # :39-41
    T = np.dtype(dataset.T).type
    flat = flatten(trees, options, dtype=T)
    nrestarts = int(getattr(options, "optimizer_nrestarts", 2))
    if noise is None:
        noise = start_noise(flat, nrestarts, rng or np.random.default_rng())
    noise = np.ascontiguousarray(noise, dtype=np.float64)
    need = int(sum(nrestarts * int(flat.const_off[i + 1] - flat.const_off[i]) for i in range(flat.ntrees)))
    if noise.shape != (need,):
        raise ValueError(f"start noise has {noise.size} values, the trees' restarts need {need}")
    par = None if loss.params is None else np.ascontiguousarray(loss.params, dtype=np.float64)
    opts = ConstOptOptions(ALGORITHMS[algorithm], int(getattr(options, "optimizer_iterations", 8)), nrestarts,
                           int(loss.kind), None if par is None else par.ctypes.data_as(C.POINTER(C.c_double)),
                           noise.ctypes.data_as(C.POINTER(C.c_double)), 0)
    consts = np.ascontiguousarray(flat.consts, dtype=T)
    tr = _trees_struct(flat, consts)
    nt = len(trees)
    out_c = np.zeros(max(consts.size, 1), dtype=T)
    out_l = np.zeros(max(nt, 1))
    out_k = np.zeros(max(nt, 1), dtype=np.uint8)
    out_n = np.zeros(max(nt, 1))
    ptrs = [a.ctypes.data_as(C.c_void_p) for a in (out_c, out_l, out_k, out_n)]
    dirs = np.ascontiguousarray([d - 1 for d in dataset.directions], dtype=np.int32)
    coef = np.ascontiguousarray(obj.coefficients, dtype=np.float64)
    dev = dataset.multi.device(device)
    check(lib().srhip_optimize_constants_deriv(dev.ctx.handle, dev.handle, C.byref(tr), C.byref(opts),
                                               dirs.ctypes.data_as(C.c_void_p), len(dirs),
                                               coef.ctypes.data_as(C.c_void_p), *ptrs))
    conv = out_k[:nt].astype(bool)
    co = flat.const_off
    for i in np.flatnonzero(conv):
        set_constants(trees[i], [T(v) for v in out_c[co[i]:co[i + 1]]])
    return ConstOptResult(out_l[:nt].copy(), conv, out_n[:nt].copy())


def _optimize_by_target(dataset, trees, options, device, evaluator_factory, noise, row_idx, tg, const_off,
                        nrestarts) -> ConstOptResult:
    """The regroup fallback of a MultiDataset: each target's trees on dataset.target(k), with the
    group's slice of the start noise (tree t's draws are noise[nrestarts·const_off[t] :
    nrestarts·const_off[t+1]]), results scattered back in the trees' order."""
    nt = len(trees)
    losses, conv, nev = np.zeros(nt), np.zeros(nt, dtype=bool), np.zeros(nt)
    co = np.asarray(const_off, dtype=np.int64) * nrestarts
    for k in np.unique(tg):
        idx = np.flatnonzero(tg == k)
        sub = np.concatenate([noise[co[t]:co[t + 1]] for t in idx]) if len(idx) else np.zeros(0)
        fac = evaluator_factory
        if fac is not None:
            try:
                takes_target = "target" in inspect.signature(fac).parameters
            except (TypeError, ValueError):
                takes_target = False
            if takes_target:
                fac = _with_target(evaluator_factory, int(k))
        r = optimize_constants_batch(dataset.target(int(k)), [trees[t] for t in idx], options, device=device,
                                     evaluator_factory=fac, noise=sub,
                                     row_idx=None if row_idx is None else row_idx[idx])
        losses[idx], conv[idx], nev[idx] = r.losses, r.converged, r.num_evals
    return ConstOptResult(losses, conv, nev)


def _with_target(factory, k: int):
    """factory with target=k bound; `members=` is passed through when the factory takes it."""
    takes_members = "members" in inspect.signature(factory).parameters
    if takes_members:
        return lambda cands, members=None: factory(cands, members=members, target=k)
    return lambda cands: factory(cands, target=k)


class _Callback:
    """srhip_constopt_eval_fn over evaluator_factory: one evaluator per member
    list the driver asks for (candidates, simplex vertices, line-search
    stragglers, the final trees), built from copies of the input trees."""

    def __init__(self, trees, factory):
        self.trees, self.factory = trees, factory
        # a factory that accepts members= is told the input tree of each candidate
        try:
            params = inspect.signature(factory).parameters.values()
            self.pass_members = any(p.name == "members" or p.kind is p.VAR_KEYWORD for p in params)
        except (TypeError, ValueError):
            self.pass_members = False
        self.cache = {}
        self.error = None
        self.fn = CONSTOPT_EVAL_FN(self._eval)

    def _eval(self, _user, n, idx, consts, grad, out_f, out_g):
        try:
            members = np.ctypeslib.as_array(idx, shape=(n,)).copy() if n else np.zeros(0, dtype=np.int32)
            key = members.tobytes()
            ev = self.cache.get(key)
            if ev is None:
                cands = [self.trees[int(i)].copy() for i in members]
                ev = self.factory(cands, members=members.copy()) if self.pass_members else self.factory(cands)
                self.cache[key] = ev
            nconst = sum(len(_consts_of(self.trees[int(i)])) for i in members)
            x = np.ctypeslib.as_array(consts, shape=(nconst,)).copy() if nconst else np.zeros(0)
            if grad:
                f, g = ev.loss_grad(x)
                if nconst:
                    np.ctypeslib.as_array(out_g, shape=(nconst,))[:] = np.asarray(g, dtype=np.float64)
            else:
                f = ev.loss_only(x)
            if n:
                np.ctypeslib.as_array(out_f, shape=(n,))[:] = np.asarray(f, dtype=np.float64)
            return 0
        except BaseException as e:  # reported after the C call returns
            self.error = e
            return 1


def _consts_of(tree: Node):
    from .node import get_constants

    return get_constants(tree)


def last_profile() -> dict:
    """Where the last optimize_constants_batch call of this thread spent its
    time (srhip_constopt_profile): seconds and call counts."""
    out = (C.c_double * 14)()
    check(lib().srhip_constopt_profile(out, 14))
    keys = ("total_s", "create_s", "set_constants_s", "loss_s", "grad_s", "kernel_s", "n_create", "n_loss", "n_grad",
            "n_rebuilt", "jit_codegen_s", "jit_load_s", "gather_s", "n_segment_evals")
    d = dict(zip(keys, (float(v) for v in out)))
    d["host_s"] = (d["total_s"] - d["create_s"] - d["set_constants_s"] - d["loss_s"] - d["grad_s"]
                   - d["gather_s"])
    return d

