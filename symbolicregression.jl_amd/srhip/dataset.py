"""`Dataset{T}` (src/Dataset.jl:24-64) with a device-resident copy.

X has the reference's shape (nfeatures, n) — X[f, i] is feature f of row i —
y is (n,), weights optional. avg_y and baseline_loss follow the reference;
the device copy (srhip_dataset) is made on first use and reused by every
evaluation (uploaded once, src/LossFunctions.jl:122-126 is the first user).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

import weakref

from .engine import DeviceDataset, MultiDeviceDataset, get_context


class Dataset:
    def __init__(self, X: np.ndarray, y: np.ndarray, weights: Optional[np.ndarray] = None,
                 varMap: Optional[Sequence[str]] = None, row_range: Optional[tuple] = None):
        X = np.asarray(X)
        y = np.asarray(y)
        if X.ndim != 2:
            raise ValueError("X must be (nfeatures, n)")
        self.X = X
        self.y = y
        self.nfeatures, self.n = X.shape
        self.weighted = weights is not None
        self.weights = None if weights is None else np.asarray(weights)
        self.varMap = list(varMap) if varMap is not None else [f"x{i + 1}" for i in range(self.nfeatures)]
        T = np.result_type(X.dtype, y.dtype)
        self.T = T.type
        # avg_y, src/Dataset.jl:56-60 (computed in T like the reference)
        if self.weighted:
            self.avg_y = T.type(np.sum(y * self.weights, dtype=T) / np.sum(self.weights, dtype=T))
        else:
            self.avg_y = T.type(np.sum(y, dtype=T) / T.type(self.n))
        self.baseline_loss = T.type(1)  # src/Dataset.jl:61
        self.row_range = row_range  # (row_begin, row_end) shard of this process, or None
        self._dev = {}

    def device(self, device: Optional[int] = None) -> DeviceDataset:
        ctx = get_context(device)
        d = self._dev.get(ctx.device)
        if d is None:
            rb, re = self.row_range if self.row_range is not None else (0, self.n)
            d = DeviceDataset(ctx, self.X, self.y, self.weights, rb, re)
            self._dev[ctx.device] = d
        return d


class _TargetDataset(Dataset):
    """Target k of a MultiDataset: a Dataset over (X, Y[k], weights[k]) whose
    device copy is a view of the parent's (no second upload of X). It holds the
    parent weakly: a view made while the parent lived keeps the device memory
    alive on its own, and without one the target uploads like any Dataset."""

    def __init__(self, parent, k: int):
        super().__init__(parent.X, parent.Y[k], None if parent.weights is None else parent.weights[k],
                         parent.varMap, parent.row_range)
        self._parent = weakref.ref(parent)
        self.target_index = k

    def device(self, device: Optional[int] = None) -> DeviceDataset:
        ctx = get_context(device)
        d = self._dev.get(ctx.device)
        if d is None:
            parent = self._parent()
            if parent is None:
                return super().device(device)
            d = parent.device(device).view(self.target_index)
            self._dev[ctx.device] = d
        return d


class MultiDataset:
    """One X (nfeatures, n) with K target rows Y (K, n) and optional per-target
    weights (K, n): what EquationSearch(X, y::AbstractMatrix) builds as nout
    Datasets over the same X (src/SymbolicRegression.jl:304-315), uploaded once.
    target(k) is an ordinary Dataset for every single-target function;
    eval_loss_batch_ok / eval_loss_batch_rowsets take the MultiDataset itself
    with one target index per tree."""

    def __init__(self, X: np.ndarray, Y: np.ndarray, weights: Optional[np.ndarray] = None,
                 varMap: Optional[Sequence[str]] = None, row_range: Optional[tuple] = None):
        X = np.asarray(X)
        Y = np.asarray(Y)
        if X.ndim != 2:
            raise ValueError("X must be (nfeatures, n)")
        W = None if weights is None else np.asarray(weights)
        if Y.ndim != 2 or Y.shape[1] != X.shape[1] or Y.shape[0] < 1 or (W is not None and W.shape != Y.shape):
            raise AssertionError("Dataset dimensions are invalid")  # Configure.jl:53-60
        self.X = X
        self.Y = Y
        self.weights = W
        self.weighted = W is not None
        self.nfeatures, self.n = X.shape
        self.ntargets = Y.shape[0]
        self.varMap = list(varMap) if varMap is not None else [f"x{i + 1}" for i in range(self.nfeatures)]
        self.row_range = row_range
        self._targets = [_TargetDataset(self, k) for k in range(self.ntargets)]
        self.T = self._targets[0].T
        self.avg_y = np.asarray([t.avg_y for t in self._targets], dtype=self.T)
        self._dev = {}

    def target(self, k: int) -> Dataset:
        if not 0 <= k < self.ntargets:
            raise IndexError("target index out of range")
        return self._targets[k]

    def device(self, device: Optional[int] = None) -> MultiDeviceDataset:
        ctx = get_context(device)
        d = self._dev.get(ctx.device)
        if d is None:
            rb, re = self.row_range if self.row_range is not None else (0, self.n)
            d = MultiDeviceDataset(ctx, self.X, self.Y, self.weights, rb, re)
            self._dev[ctx.device] = d
        return d


class DerivativeDataset(Dataset):
    """A Dataset with targets for the derivatives of the prediction as well: dydx
    (ndir, n) holds, per row, the target of ∂ŷ/∂x_d for each d of `directions`
    (1-based feature indices, as the reference's `direction::Int` of
    eval_diff_tree_array). weights is None, (n,) — shared by all channels — or
    (1 + ndir, n), channel 0 being y's. It wraps a MultiDataset with
    Y = [y; dydx], so X is stored and uploaded once: `multi` is that dataset,
    target(k) channel k as an ordinary Dataset, and the object itself is the
    Dataset over (X, y, weights of channel 0) wherever only the value is scored.
    A DerivativeObjective (options.loss_function) scores all channels."""

    def __init__(self, X: np.ndarray, y: np.ndarray, dydx: np.ndarray, directions: Sequence[int],
                 weights: Optional[np.ndarray] = None, varMap: Optional[Sequence[str]] = None):
        X = np.asarray(X)
        y = np.asarray(y)
        dydx = np.asarray(dydx)
        if X.ndim != 2:
            raise ValueError("X must be (nfeatures, n)")
        nfeat, n = X.shape
        try:
            dirs = [int(d) for d in directions]
        except TypeError:
            raise ValueError("directions must be a sequence of 1-based feature indices") from None
        if any(d != dd for d, dd in zip(dirs, directions)):
            raise ValueError("directions must be integers")
        if not 1 <= len(dirs) <= 15:
            raise ValueError("a DerivativeDataset takes 1 to 15 directions")
        if any(not 1 <= d <= nfeat for d in dirs):
            raise ValueError(f"directions must be 1-based feature indices within 1..{nfeat}")
        if len(set(dirs)) != len(dirs):
            raise ValueError("directions must not repeat")
        if y.shape != (n,):
            raise ValueError(f"y must be (n,) = ({n},), not {y.shape}")
        if dydx.shape != (len(dirs), n):
            raise ValueError(f"dydx must be (ndir, n) = ({len(dirs)}, {n}), not {dydx.shape}")
        for name, a in (("X", X), ("y", y), ("dydx", dydx)):
            if a.dtype not in (np.float32, np.float64):
                raise ValueError(f"{name} must be float32 or float64")
        if not (X.dtype == y.dtype == dydx.dtype):
            raise ValueError("X, y and dydx must have one dtype")
        W = None
        if weights is not None:
            w = np.asarray(weights)
            if w.dtype != X.dtype:
                raise ValueError("weights must have the dtype of X")
            if w.shape == (n,):
                W = np.broadcast_to(w, (1 + len(dirs), n))
            elif w.shape == (1 + len(dirs), n):
                W = w
            else:
                raise ValueError(f"weights must be (n,) or (1 + ndir, n) = ({1 + len(dirs)}, {n}), not {w.shape}")
        super().__init__(X, y, None if W is None else W[0], varMap)
        self.dydx = dydx
        self.directions = tuple(dirs)
        self.ndir = len(dirs)
        self.multi = MultiDataset(X, np.concatenate([y[None, :], dydx]), W, varMap)

    def target(self, k: int) -> Dataset:
        """Channel k (0: y; 1 + j: the derivative along directions[j]) as a Dataset."""
        return self.multi.target(k)

    def device(self, device: Optional[int] = None) -> DeviceDataset:
        return self.multi.target(0).device(device)


class GroupDataset(Dataset):
    """A Dataset whose rows are sharded over the members of a DeviceGroup
    (srhip_group_dataset), uploaded when it is made. eval_loss_batch_ok,
    eval_loss_grad_batch and optimize_constants_batch take it where they take
    a Dataset and then run over the whole group."""

    def __init__(self, group, X: np.ndarray, y: np.ndarray, weights: Optional[np.ndarray] = None,
                 varMap: Optional[Sequence[str]] = None):
        import ctypes as C

        from . import constants as K
        from ._lib import check, lib
        from .engine import DeviceGroup, dtype_code

        if not isinstance(group, DeviceGroup):
            raise TypeError("group must be a DeviceGroup")
        self.handle = None
        super().__init__(X, y, weights, varMap)
        self.group = group
        dt = np.dtype(self.T)
        if self.X.flags.c_contiguous:
            layout, Xa = K.X_FEATURE_MAJOR, np.ascontiguousarray(self.X, dtype=dt)
        else:  # Fortran order = Julia's column-major (nfeatures, n)
            layout, Xa = K.X_JULIA, np.asfortranarray(self.X, dtype=dt)
        ya = np.ascontiguousarray(self.y, dtype=dt)
        wa = None if self.weights is None else np.ascontiguousarray(self.weights, dtype=dt)
        if ya.shape != (self.n,) or (wa is not None and wa.shape != (self.n,)):
            raise AssertionError("Dataset dimensions are invalid")  # Configure.jl:53-60
        h = C.c_void_p()
        check(lib().srhip_group_dataset_create(group._live(), dtype_code(dt), layout, Xa.ctypes.data, ya.ctypes.data,
                                               None if wa is None else wa.ctypes.data, self.n, self.nfeatures,
                                               C.byref(h)))
        self.handle = h

    def device(self, device: Optional[int] = None):
        raise TypeError("a GroupDataset lives on its group's members; use group.context(k) with a Dataset for one device")

    def info(self):
        import ctypes as C

        from ._lib import check, lib

        if not self.handle:
            raise ValueError("the group dataset is closed")
        rows, nf, fin = C.c_int64(), C.c_int32(), C.c_int32()
        sw, syw = C.c_double(), C.c_double()
        check(lib().srhip_group_dataset_info(self.handle, C.byref(rows), C.byref(nf), C.byref(sw), C.byref(syw),
                                             C.byref(fin)))
        return dict(rows=rows.value, nfeat=nf.value, sum_w=sw.value, sum_yw=syw.value, x_finite=bool(fin.value))

    def close(self):
        from ._lib import lib

        if self.handle and self.group.handle:
            lib().srhip_group_dataset_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
