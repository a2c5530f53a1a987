"""Thin object layer over the C ABI: device contexts, device datasets and
compiled programs. Everything here calls libsrhip.so; nothing computes on
the CPU."""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional

import numpy as np

from . import constants as K
from ._lib import SrhipError, Trees, check, lib
from .node import FlatTrees

_ctx_lock = threading.Lock()
_contexts: dict = {}


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data  # an int: ctypes passes it as void*, cheaper than data_as


def dtype_code(dtype) -> int:
    dt = np.dtype(dtype)
    if dt == np.float32:
        return K.F32
    if dt == np.float64:
        return K.F64
    from ._lib import Unsupported

    raise Unsupported(-2, f"dtype {dt} is not supported by the engine (Float32/Float64 only)")


def device_count() -> int:
    n = C.c_int32(0)
    lib().srhip_device_count(C.byref(n))
    return n.value


class Context:
    """One device + stream (srhip_open). Calls through one context are
    serialised by the library."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check(lib().srhip_open(int(device), C.byref(h)))
        self.handle = h
        self.device = int(device)

    def close(self):
        if self.handle:
            lib().srhip_close(self.handle)
            self.handle = None

    def last_kernel_time(self):
        ms = C.c_double(0)
        n = C.c_int32(0)
        check(lib().srhip_last_kernel_time(self.handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def sync(self):
        check(lib().srhip_sync(self.handle))

    def last_bailed(self) -> int:
        """Trees of the last eval whose tree code handed a tile back."""
        return self.last_jit_events()[0]

    def last_kernel_name(self) -> str:
        """The main evaluation kernel this thread launched last (srhip_last_kernel_name)."""
        buf = C.create_string_buffer(128)
        check(lib().srhip_last_kernel_name(buf, 128))
        return buf.value.decode()

    def last_loss_launch(self):
        """Geometry of the loss tree-code launch this thread made last (srhip_last_loss_launch)."""
        v = (C.c_int32 * 6)()
        check(lib().srhip_last_loss_launch(v))
        return dict(zip(("nrg", "ntg", "tpb", "grid", "tbig", "tsub"), (int(x) for x in v)))

    def last_tree_code(self) -> int:
        """Trees the last eval ran as tree code (srhip_last_tree_code)."""
        n = C.c_int32(0)
        check(lib().srhip_last_tree_code(self.handle, C.byref(n)))
        return n.value

    def column_cache_info(self):
        """Shared-subtree columns of this context (srhip_column_cache_info):
        columns derived, columns found in a dataset's pool, derive programs
        built, slots of the registry."""
        d, r, b = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        n = C.c_int32(0)
        check(lib().srhip_column_cache_info(self.handle, C.byref(d), C.byref(r), C.byref(b), C.byref(n)))
        return dict(derived=d.value, reused=r.value, programs=b.value, nslot=n.value)

    def last_jit_events(self):
        """(trees handed back to the interpreter, tiles redone with the
        PRECISE routines) of the last eval."""
        n = C.c_int32(0)
        r = C.c_int64(0)
        check(lib().srhip_last_bailed(self.handle, C.byref(n), C.byref(r)))
        return n.value, r.value


def default_device() -> int:
    return int(os.environ.get("SRHIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def get_context(device: Optional[int] = None) -> Context:
    d = default_device() if device is None else int(device)
    with _ctx_lock:
        c = _contexts.get(d)
        if c is None:
            c = Context(d)
            _contexts[d] = c
        return c


class DeviceDataset:
    """srhip_dataset: rows [row_begin, row_end) of X (nfeatures, n), y, w
    resident on one device."""

    def __init__(self, ctx: Context, X: np.ndarray, y: np.ndarray, w: Optional[np.ndarray] = None,
                 row_begin: int = 0, row_end: Optional[int] = None):
        if X.ndim != 2:
            raise ValueError("X must be (nfeatures, n)")
        dt = np.result_type(X.dtype, y.dtype)
        code = dtype_code(dt)
        nfeat, n = X.shape
        if X.flags.c_contiguous:
            layout, Xa = K.X_FEATURE_MAJOR, np.ascontiguousarray(X, dtype=dt)
        else:  # Fortran order = Julia's column-major (nfeatures, n)
            layout, Xa = K.X_JULIA, np.asfortranarray(X, dtype=dt)
        ya = np.ascontiguousarray(y, dtype=dt)
        wa = None if w is None else np.ascontiguousarray(w, dtype=dt)
        if ya.shape != (n,) or (wa is not None and wa.shape != (n,)):
            raise AssertionError("Dataset dimensions are invalid")  # Configure.jl:53-60
        rb = int(row_begin)
        re = n if row_end is None else int(row_end)
        h = C.c_void_p()
        check(lib().srhip_dataset_create(ctx.handle, code, layout, _p(Xa), _p(ya), _p(wa), n, nfeat, rb,
                                         re, C.byref(h)))
        self.handle = h
        self.ctx = ctx
        self.dtype = dt
        self.nfeat = nfeat
        self.rows = re - rb
        self.weighted = w is not None

    def info(self):
        rows = C.c_int64()
        nf = C.c_int32()
        sw = C.c_double()
        syw = C.c_double()
        fin = C.c_int32()
        check(lib().srhip_dataset_info(self.handle, C.byref(rows), C.byref(nf), C.byref(sw), C.byref(syw),
                                       C.byref(fin)))
        return dict(rows=rows.value, nfeat=nf.value, sum_w=sw.value, sum_yw=syw.value, x_finite=bool(fin.value))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib().srhip_dataset_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class MultiDeviceDataset:
    """srhip_dataset of several targets (srhip_dataset_create_multi): rows
    [row_begin, row_end) of one X (nfeatures, n) with the target columns Y
    (ntargets, n) and optional weight columns W (ntargets, n). view(k) is target
    k as a DeviceDataset on the same device memory."""

    def __init__(self, ctx: Context, X: np.ndarray, Y: np.ndarray, W: Optional[np.ndarray] = None,
                 row_begin: int = 0, row_end: Optional[int] = None):
        if X.ndim != 2:
            raise ValueError("X must be (nfeatures, n)")
        dt = np.result_type(X.dtype, Y.dtype)
        code = dtype_code(dt)
        nfeat, n = X.shape
        if X.flags.c_contiguous:
            layout, Xa = K.X_FEATURE_MAJOR, np.ascontiguousarray(X, dtype=dt)
        else:  # Fortran order = Julia's column-major (nfeatures, n)
            layout, Xa = K.X_JULIA, np.asfortranarray(X, dtype=dt)
        Ya = np.ascontiguousarray(Y, dtype=dt)
        Wa = None if W is None else np.ascontiguousarray(W, dtype=dt)
        if Ya.ndim != 2 or Ya.shape[1] != n or (Wa is not None and Wa.shape != Ya.shape):
            raise AssertionError("Dataset dimensions are invalid")  # Configure.jl:53-60
        rb = int(row_begin)
        re = n if row_end is None else int(row_end)
        h = C.c_void_p()
        check(lib().srhip_dataset_create_multi(ctx.handle, code, layout, _p(Xa), _p(Ya), _p(Wa), n, nfeat,
                                               Ya.shape[0], rb, re, C.byref(h)))
        self.handle = h
        self.ctx = ctx
        self.dtype = dt
        self.nfeat = nfeat
        self.ntargets = Ya.shape[0]
        self.rows = re - rb
        self.weighted = W is not None

    info = DeviceDataset.info

    def target_info(self, k: int):
        """(Σw, Σ y·w) of target k over the shard (srhip_dataset_target_info)."""
        sw, syw = C.c_double(), C.c_double()
        check(lib().srhip_dataset_target_info(self.handle, int(k), C.byref(sw), C.byref(syw)))
        return sw.value, syw.value

    def view(self, k: int) -> DeviceDataset:
        """Target k as a single-target DeviceDataset sharing this dataset's
        device memory (srhip_dataset_view); it may outlive this object."""
        h = C.c_void_p()
        check(lib().srhip_dataset_view(self.handle, int(k), C.byref(h)))
        v = DeviceDataset.__new__(DeviceDataset)
        v.handle = h
        v.ctx = self.ctx
        v.dtype = self.dtype
        v.nfeat = self.nfeat
        v.rows = self.rows
        v.weighted = self.weighted
        return v

    __del__ = DeviceDataset.__del__


class Program:
    """srhip_program: a compiled, device-resident batch of trees.
    varying_constants (SRHIP_PROGRAM_VARYING_CONSTANTS): the caller will set
    new constants, so Float32 tree code reads them from memory from the start.
    wide_tree_code (SRHIP_PROGRAM_WIDE_TREE_CODE, opt-in): Float32 literal-constant
    loss tree code may read its features from X in device memory, so trees that
    read features past the LDS tile's reach (index 63 on) and datasets too wide
    for LDS keep their tree code."""

    def __init__(self, ctx: Context, flat: FlatTrees, dtype, varying_constants: bool = False,
                 interpreted: bool = False, wide_tree_code: bool = False):
        self.ctx = ctx
        self.dtype = np.dtype(dtype)
        self.flat = flat
        consts = np.ascontiguousarray(flat.consts, dtype=self.dtype)
        self._keep = (flat.node_off, flat.kind, flat.arg, flat.const_off, consts)
        tr = Trees(
            flat.ntrees,
            flat.node_off.ctypes.data_as(C.POINTER(C.c_int32)),
            flat.kind.ctypes.data_as(C.POINTER(C.c_uint8)),
            flat.arg.ctypes.data_as(C.POINTER(C.c_uint16)),
            flat.const_off.ctypes.data_as(C.POINTER(C.c_int32)),
            consts.ctypes.data_as(C.c_void_p),
        )
        h = C.c_void_p()
        check(lib().srhip_program_create_ex(ctx.handle, dtype_code(self.dtype), C.byref(tr),
                                            (K.PROGRAM_VARYING_CONSTANTS if varying_constants else 0)
                                            | (K.PROGRAM_INTERPRETED if interpreted else 0)
                                            | (K.PROGRAM_WIDE_TREE_CODE if wide_tree_code else 0), C.byref(h)))
        self.handle = h
        self.ntrees = flat.ntrees

    def info(self):
        nt = C.c_int32()
        tot = C.c_int64()
        nodes = np.zeros(max(self.ntrees, 1), dtype=np.int32)
        check(lib().srhip_program_info(self.handle, C.byref(nt), C.byref(tot), _p(nodes)))
        return nt.value, tot.value, nodes[: nt.value]

    def jit_info(self):
        """Tree code of this program (srhip_program_jit_info)."""
        nt, nf = C.c_int32(), C.c_int32()
        nb = C.c_int64()
        mc, ml = C.c_double(), C.c_double()
        check(lib().srhip_program_jit_info(self.handle, C.byref(nt), C.byref(nf), C.byref(nb), C.byref(mc),
                                           C.byref(ml)))
        return dict(ntrees=nt.value, nfast=nf.value, code_bytes=nb.value, ms_codegen=mc.value, ms_load=ml.value)

    def shared_columns(self):
        """{canonical subtree text: slot} of the L2 loss tree code's
        shared-subtree columns (srhip_program_shared_columns)."""
        n = C.c_int64(1 << 16)
        buf = C.create_string_buffer(n.value)
        check(lib().srhip_program_shared_columns(self.handle, buf, C.byref(n)))
        out = {}
        for line in buf.value.decode().splitlines():
            slot, key = line.split(" ", 1)
            out[key] = int(slot)
        return out

    def grad_jit_info(self):
        """Gradient tree code of this program (srhip_program_grad_jit_info)."""
        nt, nr = C.c_int32(), C.c_int32()
        nb = C.c_int64()
        mc, ml = C.c_double(), C.c_double()
        check(lib().srhip_program_grad_jit_info(self.handle, C.byref(nt), C.byref(nr), C.byref(nb), C.byref(mc),
                                                C.byref(ml)))
        return dict(ntrees=nt.value, nrejected=nr.value, code_bytes=nb.value, ms_codegen=mc.value,
                    ms_load=ml.value)

    def pass_info(self):
        """Which kernel passes the trees go to (srhip_program_pass_info): the evaluation lists
        and, after the first gradient call, the gradient work items per pass
        (G = 1, 2, 4 tangents, deep); opsets are "BASIC" or "FULL"."""
        ev, gi, gr = (C.c_int32 * 4)(), (C.c_int32 * 4)(), (C.c_int32 * 4)()
        go = C.c_int32()
        check(lib().srhip_program_pass_info(self.handle, ev, gi, gr, C.byref(go)))
        names = ("BASIC", "FULL")
        return dict(shallow=ev[0], deep=ev[1], tree_code=ev[2], opset=names[ev[3]], grad_items=tuple(gi),
                    grad_rest=tuple(gr), grad_opset=names[go.value])

    def update_stats(self):
        """How set_constants applied new constants: {"inplace": n, "rebuilt": n}."""
        a, b = C.c_int64(), C.c_int64()
        check(lib().srhip_program_update_stats(self.handle, C.byref(a), C.byref(b)))
        return dict(inplace=a.value, rebuilt=b.value)

    def set_constants(self, consts: np.ndarray):
        c = np.ascontiguousarray(consts, dtype=self.dtype)
        if c.shape != (int(self.flat.const_off[-1]),):
            raise ValueError("constant vector has the wrong length")
        check(lib().srhip_program_set_constants(self.handle, _p(c)))

    def eval_loss(self, ds: DeviceDataset, loss_kind: int, params=None, row_idx=None):
        nt = self.ntrees
        sums = np.empty(max(nt, 1), dtype=np.float64)  # the library writes every tree's entry
        ok = np.empty(max(nt, 1), dtype=np.uint8)
        wsum = C.c_double(0)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        idx = None if row_idx is None else np.ascontiguousarray(row_idx, dtype=np.int64)
        nidx = 0 if idx is None else len(idx)
        check(lib().srhip_eval_loss(ds.handle, self.handle, int(loss_kind), _p(par), _p(idx), nidx, _p(sums),
                                    C.byref(wsum), _p(ok)))
        return sums[:nt], wsum.value, ok[:nt].view(bool)  # 0/1 bytes: a view, no copy

    def eval_loss_rowsets(self, ds: DeviceDataset, loss_kind: int, row_idx, params=None):
        """srhip_eval_loss_rowsets: tree t on its own rows row_idx[t] (an
        (ntrees, batch_size) integer array): (Σ w·ℓ per tree, Σ w per tree, ok)."""
        nt = self.ntrees
        idx = np.ascontiguousarray(row_idx, dtype=np.int64)
        if idx.ndim != 2 or idx.shape[0] != nt:
            raise ValueError("row_idx must be (ntrees, batch_size)")
        sums = np.empty(max(nt, 1), dtype=np.float64)
        wsum = np.empty(max(nt, 1), dtype=np.float64)
        ok = np.empty(max(nt, 1), dtype=np.uint8)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_eval_loss_rowsets(ds.handle, self.handle, int(loss_kind), _p(par), _p(idx), idx.shape[1],
                                            _p(sums), _p(wsum), _p(ok)))
        return sums[:nt], wsum[:nt], ok[:nt].view(bool)

    def eval_loss_targets(self, ds, loss_kind: int, targets, params=None):
        """srhip_eval_loss_targets: tree t against column targets[t] of a
        MultiDeviceDataset in one launch: (Σ w·ℓ per tree, Σ w per target, ok)."""
        nt = self.ntrees
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        if tg.shape != (nt,):
            raise ValueError("targets must have one entry per tree")
        ntg = getattr(ds, "ntargets", 1)
        sums = np.empty(max(nt, 1), dtype=np.float64)
        wsum = np.empty(ntg, dtype=np.float64)
        ok = np.empty(max(nt, 1), dtype=np.uint8)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_eval_loss_targets(ds.handle, self.handle, int(loss_kind), _p(par), _p(tg), _p(sums),
                                            _p(wsum), _p(ok)))
        return sums[:nt], wsum, ok[:nt].view(bool)

    def eval_loss_rowsets_targets(self, ds, loss_kind: int, targets, row_idx, params=None):
        """srhip_eval_loss_rowsets_targets: tree t on its own rows row_idx[t]
        against column targets[t]: (Σ w·ℓ per tree, Σ w per tree, ok)."""
        nt = self.ntrees
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        if tg.shape != (nt,):
            raise ValueError("targets must have one entry per tree")
        idx = np.ascontiguousarray(row_idx, dtype=np.int64)
        if idx.ndim != 2 or idx.shape[0] != nt:
            raise ValueError("row_idx must be (ntrees, batch_size)")
        sums = np.empty(max(nt, 1), dtype=np.float64)
        wsum = np.empty(max(nt, 1), dtype=np.float64)
        ok = np.empty(max(nt, 1), dtype=np.uint8)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_eval_loss_rowsets_targets(ds.handle, self.handle, int(loss_kind), _p(par), _p(tg), _p(idx),
                                                    idx.shape[1], _p(sums), _p(wsum), _p(ok)))
        return sums[:nt], wsum[:nt], ok[:nt].view(bool)

    def eval_loss_packed(self, ds: DeviceDataset, loss_kind: int, d_out: int, params=None):
        """srhip_eval_loss_packed: [Σw·ℓ, failed] per tree + Σw written to the
        device buffer at address d_out (2·ntrees + 1 float64, e.g. a torch
        tensor's data_ptr()), enqueued on the context's stream (ctx.sync()
        before another stream reads it)."""
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_eval_loss_packed(ds.handle, self.handle, int(loss_kind), _p(par), C.c_void_p(int(d_out))))

    def eval_loss_grad(self, ds: DeviceDataset, loss_kind: int, params=None):
        """(Σ w·ℓ per tree, Σ w·∂ℓ/∂c per constant [const_off order], Σw, ok)."""
        nt = self.ntrees
        nc = int(self.flat.const_off[-1])
        sums = np.zeros(max(nt, 1), dtype=np.float64)
        grads = np.zeros(max(nc, 1), dtype=np.float64)
        ok = np.zeros(max(nt, 1), dtype=np.uint8)
        wsum = C.c_double(0)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_eval_loss_grad(ds.handle, self.handle, int(loss_kind), _p(par), _p(sums), _p(grads),
                                         C.byref(wsum), _p(ok)))
        return sums[:nt], grads[:nc], wsum.value, ok[:nt].astype(bool)

    def eval_loss_grad_rowsets(self, ds: DeviceDataset, loss_kind: int, row_idx, params=None):
        """srhip_eval_loss_grad_rowsets: tree t on its own rows row_idx[t] (an
        (ntrees, batch_size) integer array): (Σ w·ℓ per tree, Σ w·∂ℓ/∂c per
        constant [const_off order], Σ w per tree, ok)."""
        nt = self.ntrees
        nc = int(self.flat.const_off[-1])
        idx = np.ascontiguousarray(row_idx, dtype=np.int64)
        if idx.ndim != 2 or idx.shape[0] != nt:
            raise ValueError("row_idx must be (ntrees, batch_size)")
        sums = np.zeros(max(nt, 1), dtype=np.float64)
        grads = np.zeros(max(nc, 1), dtype=np.float64)
        wsum = np.zeros(max(nt, 1), dtype=np.float64)
        ok = np.zeros(max(nt, 1), dtype=np.uint8)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_eval_loss_grad_rowsets(ds.handle, self.handle, int(loss_kind), _p(par), _p(idx), idx.shape[1],
                                                 _p(sums), _p(grads), _p(wsum), _p(ok)))
        return sums[:nt], grads[:nc], wsum[:nt], ok[:nt].astype(bool)

    def eval_loss_grad_targets(self, ds, loss_kind: int, targets, params=None):
        """srhip_eval_loss_grad_targets: tree t against column targets[t] of a
        MultiDeviceDataset in one launch per pass: (Σ w·ℓ per tree, Σ w·∂ℓ/∂c per
        constant [const_off order], Σ w per target, ok)."""
        nt = self.ntrees
        nc = int(self.flat.const_off[-1])
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        if tg.shape != (nt,):
            raise ValueError("targets must have one entry per tree")
        ntg = getattr(ds, "ntargets", 1)
        sums = np.zeros(max(nt, 1), dtype=np.float64)
        grads = np.zeros(max(nc, 1), dtype=np.float64)
        wsum = np.zeros(ntg, dtype=np.float64)
        ok = np.zeros(max(nt, 1), dtype=np.uint8)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_eval_loss_grad_targets(ds.handle, self.handle, int(loss_kind), _p(par), _p(tg), _p(sums),
                                                 _p(grads), _p(wsum), _p(ok)))
        return sums[:nt], grads[:nc], wsum, ok[:nt].astype(bool)

    def eval_loss_deriv(self, ds, loss_kind: int, directions, params=None):
        """srhip_eval_loss_deriv: one table loss on ŷ and on ∂ŷ/∂x_d for every d of
        directions (0-based feature indices), over a MultiDeviceDataset whose columns
        are y and one target per direction: (Σ w·ℓ [ntrees, 1 + ndir], Σ w per column
        [1 + ndir], ok). A failed tree's row is NaN; a non-finite derivative leaves
        ok set and its channel non-finite."""
        nt = self.ntrees
        d = np.ascontiguousarray(directions, dtype=np.int32)
        if d.ndim != 1:
            raise ValueError("directions must be a list of feature indices")
        nd = len(d)
        sums = np.zeros((max(nt, 1), 1 + nd), dtype=np.float64)
        wsum = np.zeros(1 + nd, dtype=np.float64)
        ok = np.zeros(max(nt, 1), dtype=np.uint8)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_eval_loss_deriv(ds.handle, self.handle, int(loss_kind), _p(par), _p(d) if nd else None, nd,
                                          _p(sums), _p(wsum), _p(ok)))
        return sums[:nt], wsum, ok[:nt].astype(bool)

    def eval_loss_grad_deriv(self, ds, loss_kind: int, directions, params=None):
        """srhip_eval_loss_grad_deriv: eval_loss_deriv's sums and their derivatives with
        respect to every constant, in one launch: (Σ w·ℓ [ntrees, 1 + ndir], Σ w·ℓ'·∂/∂c
        [total consts, 1 + ndir] — column 0 through ∂ŷ/∂c, column 1 + k through
        ∂²ŷ/∂x_d∂c — Σ w per column [1 + ndir], ok). A failed tree's rows are NaN."""
        nt = self.ntrees
        nc = int(self.flat.const_off[-1])
        d = np.ascontiguousarray(directions, dtype=np.int32)
        if d.ndim != 1:
            raise ValueError("directions must be a list of feature indices")
        nd = len(d)
        sums = np.zeros((max(nt, 1), 1 + nd), dtype=np.float64)
        grads = np.zeros((max(nc, 1), 1 + nd), dtype=np.float64)
        wsum = np.zeros(1 + nd, dtype=np.float64)
        ok = np.zeros(max(nt, 1), dtype=np.uint8)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_eval_loss_grad_deriv(ds.handle, self.handle, int(loss_kind), _p(par), _p(d) if nd else None,
                                               nd, _p(sums), _p(grads), _p(wsum), _p(ok)))
        return sums[:nt], grads[:nc], wsum, ok[:nt].astype(bool)

    def eval_mixed_tree_array(self, ds, directions):
        """srhip_eval_mixed_tree_array: (∂ŷ/∂x_d [ntrees, ndir, rows], ∂²ŷ/∂x_d∂c
        [total consts, ndir, rows], ok) for every d of directions (0-based)."""
        nt = self.ntrees
        nc = int(self.flat.const_off[-1])
        d = np.ascontiguousarray(directions, dtype=np.int32)
        if d.ndim != 1:
            raise ValueError("directions must be a list of feature indices")
        nd = len(d)
        der = np.empty((nt, nd, ds.rows), dtype=self.dtype)
        mix = np.empty((nc, nd, ds.rows), dtype=self.dtype)
        ok = np.zeros(max(nt, 1), dtype=np.uint8)
        check(lib().srhip_eval_mixed_tree_array(ds.handle, self.handle, _p(d) if nd else None, nd, _p(der), _p(mix),
                                                _p(ok)))
        return der, mix, ok[:nt].astype(bool)

    def eval_loss_grad_rowsets_targets(self, ds, loss_kind: int, targets, row_idx, params=None):
        """srhip_eval_loss_grad_rowsets_targets: tree t on its own rows row_idx[t]
        against column targets[t]: (Σ w·ℓ per tree, Σ w·∂ℓ/∂c per constant, Σ w per
        tree, ok)."""
        nt = self.ntrees
        nc = int(self.flat.const_off[-1])
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        if tg.shape != (nt,):
            raise ValueError("targets must have one entry per tree")
        idx = np.ascontiguousarray(row_idx, dtype=np.int64)
        if idx.ndim != 2 or idx.shape[0] != nt:
            raise ValueError("row_idx must be (ntrees, batch_size)")
        sums = np.zeros(max(nt, 1), dtype=np.float64)
        grads = np.zeros(max(nc, 1), dtype=np.float64)
        wsum = np.zeros(max(nt, 1), dtype=np.float64)
        ok = np.zeros(max(nt, 1), dtype=np.uint8)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_eval_loss_grad_rowsets_targets(ds.handle, self.handle, int(loss_kind), _p(par), _p(tg),
                                                         _p(idx), idx.shape[1], _p(sums), _p(grads), _p(wsum),
                                                         _p(ok)))
        return sums[:nt], grads[:nc], wsum[:nt], ok[:nt].astype(bool)

    def eval_grad_tree_array(self, ds: DeviceDataset):
        """(ŷ [ntrees][rows], ∂ŷ/∂c [total consts][rows], ok)."""
        nt = self.ntrees
        nc = int(self.flat.const_off[-1])
        val = np.empty((nt, ds.rows), dtype=self.dtype)
        grad = np.empty((nc, ds.rows), dtype=self.dtype)
        ok = np.zeros(max(nt, 1), dtype=np.uint8)
        check(lib().srhip_eval_grad_tree_array(ds.handle, self.handle, _p(val), _p(grad), _p(ok)))
        return val, grad, ok[:nt].astype(bool)

    def eval_tree_array(self, ds: DeviceDataset):
        nt = self.ntrees
        out = np.empty((nt, ds.rows), dtype=self.dtype)
        ok = np.zeros(max(nt, 1), dtype=np.uint8)
        check(lib().srhip_eval_tree_array(ds.handle, self.handle, _p(out), _p(ok)))
        return out, ok[:nt].astype(bool)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                lib().srhip_program_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class _MemberContext(Context):
    """Member k's context of a DeviceGroup, lent (srhip_group_ctx): the group
    owns it, so close() leaves it open."""

    def __init__(self, handle, device: int):
        self.handle = handle
        self.device = int(device)

    def close(self):
        self.handle = None


def group_shard_range(n: int, ndev: int, k: int):
    """srhip_group_shard_range: rows [begin, end) of member k of ndev."""
    b, e = C.c_int64(0), C.c_int64(0)
    check(lib().srhip_group_shard_range(int(n), int(ndev), int(k), C.byref(b), C.byref(e)))
    return b.value, e.value


class DeviceGroup:
    """srhip_group: one process, one member (context + driver thread) per entry
    of `devices`; the same device may be listed more than once. Datasets are
    row-sharded over the members, programs are built on every member, and one
    evaluation call combines the shards on the device in member order.
    A context manager; closing it first destroys the datasets and programs
    made through it that are still alive."""

    def __init__(self, devices):
        try:
            devs = [int(d) for d in devices]
        except TypeError:
            raise TypeError("devices must be a sequence of device indices") from None
        if not 1 <= len(devs) <= 16:
            raise ValueError("a device group has 1 to 16 members")
        if any(d < 0 for d in devs):
            raise ValueError("device indices are non-negative")
        self.handle = None
        self._children = []
        arr = (C.c_int32 * len(devs))(*devs)
        h = C.c_void_p()
        check(lib().srhip_group_open(arr, len(devs), C.byref(h)))
        self.handle = h
        self.devices = tuple(devs)
        self.ndev = len(devs)

    def _live(self):
        if not self.handle:
            raise ValueError("the device group is closed")
        return self.handle

    def _adopt(self, child):
        import weakref

        self._children = [r for r in self._children if r() is not None]
        self._children.append(weakref.ref(child))
        return child

    def dataset(self, X, y, weights=None):
        """A GroupDataset: rows of (X (nfeatures, n), y, weights) sharded over the members."""
        from .dataset import GroupDataset

        return self._adopt(GroupDataset(self, X, y, weights))

    def program(self, flat: FlatTrees, dtype, flags: int = 0, wide_tree_code: bool = False):
        """A GroupProgram: the trees compiled on every member (flags: PROGRAM_*;
        wide_tree_code: PROGRAM_WIDE_TREE_CODE among them)."""
        return self._adopt(GroupProgram(self, flat, dtype, flags, wide_tree_code=wide_tree_code))

    def context(self, k: int) -> Context:
        """Member k's context, for the single-device calls of an island on device k."""
        h = C.c_void_p()
        check(lib().srhip_group_ctx(self._live(), int(k), C.byref(h)))
        return _MemberContext(h, self.devices[int(k)])

    def info(self):
        n = C.c_int32(0)
        devs = (C.c_int32 * 16)()
        check(lib().srhip_group_info(self._live(), C.byref(n), devs))
        return tuple(devs[: n.value])

    def close(self):
        if not self.handle:
            return
        for r in self._children:
            c = r()
            if c is not None:
                c.close()
        self._children = []
        lib().srhip_group_close(self.handle)
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GroupProgram:
    """srhip_group_program: one identical program per member of a DeviceGroup."""

    def __init__(self, group: DeviceGroup, flat: FlatTrees, dtype, flags: int = 0, wide_tree_code: bool = False):
        if wide_tree_code:
            flags = int(flags) | K.PROGRAM_WIDE_TREE_CODE
        if not isinstance(group, DeviceGroup):
            raise TypeError("group must be a DeviceGroup")
        if not isinstance(flat, FlatTrees):
            raise TypeError("flat must be FlatTrees (srhip.flatten)")
        self.handle = None
        self.group = group
        self.dtype = np.dtype(dtype)
        self.flat = flat
        consts = np.ascontiguousarray(flat.consts, dtype=self.dtype)
        tr = _trees_struct(flat, consts)
        h = C.c_void_p()
        check(lib().srhip_group_program_create(group._live(), dtype_code(self.dtype), C.byref(tr), int(flags),
                                               C.byref(h)))
        self.handle = h
        self.ntrees = flat.ntrees

    def _gds(self, gds):
        if not hasattr(gds, "group") or not getattr(gds, "handle", None):
            raise TypeError("a GroupProgram is evaluated on a live GroupDataset")
        if not self.handle:
            raise ValueError("the group program is closed")
        return gds.handle

    def set_constants(self, consts: np.ndarray):
        c = np.ascontiguousarray(consts, dtype=self.dtype)
        if c.shape != (int(self.flat.const_off[-1]),):
            raise ValueError("constant vector has the wrong length")
        if not self.handle:
            raise ValueError("the group program is closed")
        check(lib().srhip_group_program_set_constants(self.handle, _p(c)))

    def eval_loss(self, gds, loss_kind: int, params=None):
        """(Σ w·ℓ per tree, Σw, ok) over all rows of all shards."""
        nt = self.ntrees
        sums = np.empty(max(nt, 1), dtype=np.float64)
        ok = np.empty(max(nt, 1), dtype=np.uint8)
        wsum = C.c_double(0)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_group_eval_loss(self._gds(gds), self.handle, int(loss_kind), _p(par), _p(sums),
                                          C.byref(wsum), _p(ok)))
        return sums[:nt], wsum.value, ok[:nt].view(bool)

    def eval_loss_grad(self, gds, loss_kind: int, params=None):
        """(Σ w·ℓ per tree, Σ w·∂ℓ/∂c per constant [const_off order], Σw, ok)."""
        nt = self.ntrees
        nc = int(self.flat.const_off[-1])
        sums = np.zeros(max(nt, 1), dtype=np.float64)
        grads = np.zeros(max(nc, 1), dtype=np.float64)
        ok = np.zeros(max(nt, 1), dtype=np.uint8)
        wsum = C.c_double(0)
        par = None if params is None else np.asarray(params, dtype=np.float64)
        check(lib().srhip_group_eval_loss_grad(self._gds(gds), self.handle, int(loss_kind), _p(par), _p(sums),
                                               _p(grads), C.byref(wsum), _p(ok)))
        return sums[:nt], grads[:nc], wsum.value, ok[:nt].astype(bool)

    def close(self):
        if self.handle and self.group.handle:
            lib().srhip_group_program_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _trees_struct(flat: FlatTrees, consts: np.ndarray) -> Trees:
    return Trees(
        flat.ntrees,
        flat.node_off.ctypes.data_as(C.POINTER(C.c_int32)),
        flat.kind.ctypes.data_as(C.POINTER(C.c_uint8)),
        flat.arg.ctypes.data_as(C.POINTER(C.c_uint16)),
        flat.const_off.ctypes.data_as(C.POINTER(C.c_int32)),
        consts.ctypes.data_as(C.c_void_p),
    )


def jit_compile(flat: FlatTrees, fast: bool = True, grad: bool = False, memc: bool = False, loss=None,
                out: bool = False, text: bool = True, wide: bool = False):
    """Tree compiler without a device (srhip_jit_compile, or with grad=True
    srhip_jit_compile_grad: the reverse-mode gradient tree code; memc: the
    memory-constant loss tree code; loss: a Loss other than L2, through
    srhip_jit_compile_loss; out: the per-row output code of
    srhip_eval_tree_array; wide: Float32 literal-constant loss code that
    reads its features from X in device memory): (code bytes, assembly text,
    {tree id: byte offset})."""
    f64 = np.dtype(flat.consts.dtype) == np.float64
    consts = np.ascontiguousarray(flat.consts, dtype=np.float64 if f64 else np.float32)
    tr = _trees_struct(flat, consts)
    nb, nt, no = C.c_int64(0), C.c_int64(0), C.c_int64(0)

    def call(*bufs):
        if f64 and grad:  # the Float64 gradient tree code (jit64.cpp GradGen64)
            kind, param = (0, 0.0) if loss is None else (int(loss.kind), float(loss.param))
            return lib().srhip_jit_compile_loss(C.byref(tr), 1, 8, kind, param, bufs[0], C.byref(nb), bufs[1],
                                                C.byref(nt), bufs[2], C.byref(no))
        if f64 and loss is not None:  # the Float64 tree compiler with another loss's tail
            return lib().srhip_jit_compile_loss(C.byref(tr), 0, 8, int(loss.kind), float(loss.param),
                                                bufs[0], C.byref(nb), bufs[1], C.byref(nt), bufs[2], C.byref(no))
        if f64:  # the Float64 tree compiler (jit64.cpp), L2 or per-row outputs
            return lib().srhip_jit_compile(C.byref(tr), 8 | (4 if out else 0), bufs[0], C.byref(nb), bufs[1],
                                           C.byref(nt), bufs[2], C.byref(no))
        if loss is not None:
            return lib().srhip_jit_compile_loss(C.byref(tr), int(grad), int(fast) | (32 if wide and not grad else 0),
                                                int(loss.kind), float(loss.param),
                                                bufs[0], C.byref(nb), bufs[1], C.byref(nt), bufs[2], C.byref(no))
        if grad:
            return lib().srhip_jit_compile_grad(C.byref(tr), bufs[0], C.byref(nb), bufs[1], C.byref(nt), bufs[2],
                                                C.byref(no))
        return lib().srhip_jit_compile(C.byref(tr), int(fast) | (2 if memc else 0) | (4 if out else 0) |
                                       (0 if text else 16) | (32 if wide else 0), bufs[0],
                                       C.byref(nb), bufs[1],
                                       C.byref(nt), bufs[2], C.byref(no))

    rc = call(None, None, None)
    if rc != -1:
        check(rc)
    buf = np.zeros(max(nb.value, 1), dtype=np.uint8)
    txt = C.create_string_buffer(max(nt.value, 1))
    offs = np.zeros(max(no.value, 1), dtype=np.int32)
    check(call(_p(buf), txt, _p(offs)))
    pairs = offs[: no.value].reshape(-1, 2)
    return bytes(buf[: nb.value]), txt.value.decode(), {int(t): int(o) for t, o in pairs}


def debug_constant_map(flat: FlatTrees, new_consts, dtype, grad: bool = False, keep_layout: bool = False):
    """srhip_debug_constant_map (no device): (trees that differ from a fresh
    compile after writing new_consts through the constant map, trees the
    update recompiled, 1 if it needed a rebuild). keep_layout: the images of
    a program whose constants change (failing trees keep their code)."""
    dt = np.dtype(dtype)
    consts = np.ascontiguousarray(flat.consts, dtype=dt)
    new = np.ascontiguousarray(new_consts, dtype=dt)
    tr = _trees_struct(flat, consts)
    mm, rc, rl = C.c_int64(), C.c_int64(), C.c_int32()
    check(lib().srhip_debug_constant_map(C.byref(tr), dtype_code(dt), int(grad) | (2 if keep_layout else 0), _p(new),
                                         C.byref(mm), C.byref(rc),
                                         C.byref(rl)))
    return mm.value, rc.value, rl.value


__all__ = ["Context", "DeviceDataset", "Program", "get_context", "device_count", "SrhipError", "jit_compile",
           "debug_constant_map", "DeviceGroup", "GroupProgram", "group_shard_range"]
