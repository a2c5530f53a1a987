"""Multi-output datasets, the parts that need no device: srhip.MultiDataset's shape rules
and per-target avg_y, the target-count rule of srhip_dataset_create_multi (answered before
the context is looked at), and the Julia binding's new calls against the header, with the
parsing of tests/test_julia_binding.py."""
import ctypes as C
import re

import numpy as np
import pytest

import srhip
from srhip import _lib
from srhip import constants as K
from test_julia_binding import BATCHED, HDR, JL, _c_kind, _jl_kind, header_prototypes, julia_ccalls

NEW_CALLS = ("srhip_dataset_create_multi", "srhip_dataset_view", "srhip_eval_loss_batch_targets_ctx",
             "srhip_eval_loss_rowsets_targets")
NEW_SYMBOLS = NEW_CALLS + ("srhip_dataset_targets", "srhip_dataset_target_info", "srhip_eval_loss_targets")


def data(T=np.float32, n=40, k=3):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((4, n)).astype(T)
    Y = rng.standard_normal((k, n)).astype(T)
    W = np.abs(rng.standard_normal((k, n))).astype(T)
    return X, Y, W


def test_multidataset_shape_errors():
    X, Y, W = data()
    for bad_Y, bad_W in ((Y[0], None), (Y[:, :-1], None), (Y.T, None), (Y, W[0]), (Y, W[:2]), (Y, W[:, :-1]),
                         (Y[:0], None)):
        with pytest.raises(AssertionError, match="Dataset dimensions are invalid"):
            srhip.MultiDataset(X, bad_Y, weights=bad_W)
    with pytest.raises(ValueError):
        srhip.MultiDataset(X[0], Y)
    mds = srhip.MultiDataset(X, Y, weights=W)
    assert mds.ntargets == 3 and mds.n == 40 and mds.nfeatures == 4 and mds.T == np.float32
    with pytest.raises(IndexError):
        mds.target(3)


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_per_target_avg_y_and_weights(T):
    X, Y, W = data(T)
    for weights in (None, W):
        mds = srhip.MultiDataset(X, Y, weights=weights)
        assert mds.avg_y.shape == (3,) and mds.avg_y.dtype == T
        for k in range(3):
            ref = srhip.Dataset(X, Y[k], weights=None if weights is None else W[k])
            t = mds.target(k)
            assert isinstance(t, srhip.Dataset)
            assert t.avg_y == ref.avg_y and mds.avg_y[k] == ref.avg_y and type(t.avg_y) is type(ref.avg_y)
            assert t.weighted == ref.weighted and np.array_equal(t.y, Y[k])
            assert (t.weights is None) if weights is None else np.array_equal(t.weights, W[k])
            assert t.X is mds.X  # one X on the host too


@pytest.mark.parametrize("ntargets", [0, 17, -1])
def test_target_count_is_answered_without_a_device(ntargets):
    X, Y, W = data()
    out = C.c_void_p(123)
    rc = _lib.lib().srhip_dataset_create_multi(None, K.F32, K.X_FEATURE_MAJOR, X.ctypes.data, Y.ctypes.data, None,
                                               X.shape[1], X.shape[0], ntargets, 0, X.shape[1], C.byref(out))
    assert rc == _lib.ERR_INVALID
    assert "ntargets" in _lib.lib().srhip_last_error().decode()
    assert out.value == 123  # nothing written


def test_null_Y_is_invalid_without_a_device():
    X, Y, W = data()
    out = C.c_void_p()
    rc = _lib.lib().srhip_dataset_create_multi(None, K.F32, K.X_FEATURE_MAJOR, X.ctypes.data, None, None,
                                               X.shape[1], X.shape[0], 3, 0, X.shape[1], C.byref(out))
    assert rc == _lib.ERR_INVALID and "Y" in _lib.lib().srhip_last_error().decode()


def test_header_constant_and_python_signatures():
    hdr = HDR.read_text()
    assert re.search(r"#define SRHIP_MAX_TARGETS 16\b", hdr)
    assert re.search(r"#define SRHIP_ABI_VERSION\s+1\b", hdr)
    protos = header_prototypes()
    for name in NEW_SYMBOLS:
        assert name in protos, name
        assert len(_lib.SIGNATURES[name]) == len(protos[name][1]), name
        assert hasattr(_lib.lib(), name), name
    assert "Not in this version: fused gradients" in hdr and "multi-target group datasets" in hdr


def test_every_new_ccall_matches_the_header():
    protos = header_prototypes()
    seen = set()
    for name, ret, argtypes, args in julia_ccalls():
        if name not in NEW_SYMBOLS:
            continue
        seen.add(name)
        cret, cparams = protos[name]
        assert ret == "Int32" and cret == "int32_t", name
        assert len(argtypes) == len(cparams) == len(args), name
        for jt, cp in zip(argtypes, cparams):
            assert _jl_kind(jt) == _c_kind(cp), f"{name}: Julia {jt} vs C {cp}"
    assert seen == set(NEW_CALLS), set(NEW_CALLS) ^ seen
    src = JL.read_text()
    assert int(re.search(r"const SRHIP_MAX_TARGETS = Int32\((\d+)\)", src).group(1)) == 16


def test_multicopy_checks_x_identity_and_is_held_weakly():
    src = JL.read_text()
    assert re.search(r"mutable struct MultiCopy", src)
    assert re.search(r"const MULTI_DATASETS = WeakKeyDict\{Dataset,", src)
    body = re.search(r"function MultiCopy\(.*?\nend", src, re.S).group(0)
    assert "d.X === d1.X || throw(ArgumentError" in body
    assert "finalizer(free!, m)" in body and "srhip_dataset_create_multi" in body and "srhip_dataset_view" in body
    assert "lock(CTX_LOCK) do" in body
    free = re.search(r"function free!\(m::MultiCopy\).*?\nend", src, re.S).group(0)
    assert "destroy_dataset(m.h)" in free and "m.h = C_NULL" in free and "m.views" in free
    # device_dataset hands out the view of a covered Dataset: one X per nout-output search
    dd = re.search(r"function device_dataset\(.*?\nend", src, re.S).group(0)
    assert "covering(dataset, device)" in dd and "views[" in dd
    for fn in ("eval_loss_batch_targets", "eval_loss_batch_targets_rowsets"):
        assert re.search(rf"^function {fn}\(", src, re.M), fn
    code = "\n".join(ln.split("#")[0] for ln in BATCHED.read_text().splitlines())
    multi = re.search(r"function score_batch_multi\(.*?\nend", code, re.S).group(0)
    assert "SRHip.eval_loss_batch_targets(" in multi and "SRHip.eval_loss_batch_targets_rowsets(" in multi
    assert "e isa SRHip.Unsupported || rethrow()" in multi
    assert "score_batch(datasets[j]" in multi and "score_batch_minibatch(datasets[j]" in multi


def test_targets_argument_rules_need_no_device():
    X, Y, W = data()
    o = srhip.Options(binary_operators=["+", "*"], unary_operators=["cos"])
    trees = srhip.random_population(4, o, 4, np.float32, seed=1)
    mds = srhip.MultiDataset(X, Y)
    with pytest.raises(ValueError, match="targets="):
        srhip.eval_loss_batch_ok(trees, mds, o)
    with pytest.raises(ValueError):
        srhip.eval_loss_batch_ok(trees, mds, o, targets=[0, 1, 2])
    with pytest.raises(ValueError):
        srhip.eval_loss_batch_ok(trees, mds, o, targets=[0, 1, 2, 3])
    with pytest.raises(ValueError):
        srhip.eval_loss_batch_ok(trees, srhip.Dataset(X, Y[0]), o, targets=[0, 0, 0, 0])
