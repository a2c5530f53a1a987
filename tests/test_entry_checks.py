"""The argument checks the entry points answer before they touch a device or
dereference a handle: return code and the whole srhip_last_error() text, as
recorded from the library before the runtime's repeated plumbing was folded. No
device, no dataset, no program: every call here ends in its first checks."""
import ctypes as C

import pytest

from srhip import _lib

INVALID = _lib.ERR_INVALID


def _trees(const_off):
    """One tree of one constant node; const_off as given."""
    keep = dict(
        node_off=(C.c_int32 * 2)(0, 1),
        kind=(C.c_uint8 * 1)(0),
        arg=(C.c_uint16 * 1)(0),
        const_off=(C.c_int32 * 2)(*const_off),
        consts=(C.c_double * 2)(1.0, 2.0),
    )
    t = _lib.Trees()
    t.ntrees = 1
    t.node_off = C.cast(keep["node_off"], C.POINTER(C.c_int32))
    t.kind = C.cast(keep["kind"], C.POINTER(C.c_uint8))
    t.arg = C.cast(keep["arg"], C.POINTER(C.c_uint16))
    t.const_off = C.cast(keep["const_off"], C.POINTER(C.c_int32))
    t.consts = C.cast(keep["consts"], C.c_void_p)
    return t, keep


@_lib.CONSTOPT_EVAL_FN
def _never_called(user, n, members, x, grad, f, g):
    return 1


def _multi(L, ntargets, Y):
    out = C.c_void_p()
    return L.srhip_dataset_create_multi(None, 0, 0, None, Y, None, 8, 1, ntargets, 0, 8, C.byref(out))


def _cb(L, const_off, fn, opts):
    t, keep = _trees(const_off)
    return L.srhip_optimize_constants_cb(C.byref(t), 1, opts, fn, None, None, None, None, None)


_Y = (C.c_float * 8)()
_N64 = [C.c_int64(0) for _ in range(3)]
_OPTS = _lib.ConstOptOptions()

# name -> (call, return code, message)
CASES = {
    "open_null_out": (lambda L: L.srhip_open(0, None), INVALID, "out_ctx is null"),
    "multi_ntargets_0": (lambda L: _multi(L, 0, _Y), INVALID, "ntargets must be 1..16"),
    "multi_ntargets_17": (lambda L: _multi(L, 17, _Y), INVALID, "ntargets must be 1..16"),
    "multi_null_Y": (lambda L: _multi(L, 1, None), INVALID, "null Y"),
    "batch_null_ds": (lambda L: L.srhip_eval_loss_batch(None, None, 0, None, None, 0, None, None, None),
                      INVALID, "null dataset"),
    "batch_ctx_null_ds": (lambda L: L.srhip_eval_loss_batch_ctx(None, None, None, 0, None, None, 0, None, None, None),
                          INVALID, "null dataset"),
    "batch_rowsets_ctx_null_ds": (
        lambda L: L.srhip_eval_loss_batch_rowsets_ctx(None, None, None, 0, None, None, 4, None, None, None),
        INVALID, "null dataset"),
    "batch_targets_ctx_null_ds": (
        lambda L: L.srhip_eval_loss_batch_targets_ctx(None, None, None, 0, None, None, None, None, None),
        INVALID, "null dataset"),
    "optimize_batch_null_ds": (
        lambda L: L.srhip_optimize_constants_batch(None, None, None, C.byref(_OPTS), None, None, None, None),
        INVALID, "null dataset"),
    "optimize_rowsets_null_ds": (
        lambda L: L.srhip_optimize_constants_rowsets(None, None, None, C.byref(_OPTS), None, 4, None, None, None, None),
        INVALID, "null dataset"),
    "optimize_cb_null_evaluator": (lambda L: _cb(L, (0, 1), _lib.CONSTOPT_EVAL_FN(), C.byref(_OPTS)), INVALID,
                                   "null evaluator"),
    "optimize_cb_null_options": (lambda L: _cb(L, (0, 1), _never_called, None), INVALID, "null options"),
    "optimize_cb_const_off": (lambda L: _cb(L, (1, 2), _never_called, C.byref(_OPTS)), INVALID,
                              "const_off[0] must be 0"),
    "shard_range_ndev_0": (lambda L: L.srhip_group_shard_range(10, 0, 0, C.byref(_N64[0]), C.byref(_N64[1])), INVALID,
                           "shard range: need n >= 0, 1 <= ndev <= 16 and 0 <= k < ndev"),
    "shard_range_ndev_17": (lambda L: L.srhip_group_shard_range(10, 17, 0, C.byref(_N64[0]), C.byref(_N64[1])), INVALID,
                            "shard range: need n >= 0, 1 <= ndev <= 16 and 0 <= k < ndev"),
    "jit_compile_null_trees": (
        lambda L: L.srhip_jit_compile(None, 0, None, C.byref(_N64[0]), None, C.byref(_N64[1]), None, C.byref(_N64[2])),
        INVALID, "null argument"),
    "jit_compile_grad_null_trees": (
        lambda L: L.srhip_jit_compile_grad(None, None, C.byref(_N64[0]), None, C.byref(_N64[1]), None, C.byref(_N64[2])),
        INVALID, "null argument"),
    "jit_compile_loss_null_trees": (
        lambda L: L.srhip_jit_compile_loss(None, 0, 0, 0, 0.0, None, C.byref(_N64[0]), None, C.byref(_N64[1]), None,
                                           C.byref(_N64[2])),
        INVALID, "null argument"),
    "program_info_null": (lambda L: L.srhip_program_info(None, None, None, None), INVALID, "null program"),
    "program_jit_info_null": (lambda L: L.srhip_program_jit_info(None, None, None, None, None, None), INVALID,
                              "null program"),
    "program_grad_jit_info_null": (lambda L: L.srhip_program_grad_jit_info(None, None, None, None, None, None), INVALID,
                                   "null program"),
    "program_pass_info_null": (lambda L: L.srhip_program_pass_info(None, None, None, None, None), INVALID,
                               "null program"),
    "program_update_stats_null": (lambda L: L.srhip_program_update_stats(None, None, None), INVALID, "null program"),
    "last_tree_code_null": (lambda L: L.srhip_last_tree_code(None, None), INVALID, "null argument"),
    "constopt_profile_null": (lambda L: L.srhip_constopt_profile(None, 14), INVALID, "null output"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_check_is_answered_as_before_the_folds(name):
    call, code, message = CASES[name]
    L = _lib.lib()
    rc = call(L)
    text = L.srhip_last_error().decode()
    print(name, rc, repr(text))
    assert rc == code
    assert text == message


def test_device_count_with_null_out():
    """A null out_count is allowed; without a device the call says so."""
    L = _lib.lib()
    rc = L.srhip_device_count(None)
    text = L.srhip_last_error().decode()
    print(rc, repr(text))
    assert rc in (_lib.OK, _lib.ERR_DEVICE)
    if rc == _lib.ERR_DEVICE:
        assert text == "no HIP device available"
