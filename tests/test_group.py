"""Device groups without a device (include/srhip.h "device groups"): the exported symbols and
their arities, the shard arithmetic, the argument checks that are answered before any device
is touched, the Python classes, and — statically, as tests/test_julia_binding.py does for the
rest of the binding — the Julia side: the new ccalls against the header and the `device`
keyword through BatchedCallers.jl."""
import ctypes as C
import re

import numpy as np
import pytest

import srhip
from srhip import _lib
from srhip.distributed import shard_range
from test_julia_binding import BATCHED, JL, _c_kind, _jl_kind, header_prototypes, julia_ccalls

GROUP_SYMBOLS = {
    "srhip_group_open": 3, "srhip_group_close": 1, "srhip_group_info": 3, "srhip_group_ctx": 3,
    "srhip_group_shard_range": 5, "srhip_group_dataset_create": 9, "srhip_group_dataset_destroy": 1,
    "srhip_group_dataset_info": 6, "srhip_group_program_create": 5, "srhip_group_program_destroy": 1,
    "srhip_group_program_set_constants": 2, "srhip_group_eval_loss": 7, "srhip_group_eval_loss_grad": 8,
    "srhip_group_optimize_constants": 7,
}

# the BatchedCallers.jl functions that end in an SRHip call
DEVICE_FUNCTIONS = ("score_batch", "score_batch_minibatch", "population_batched", "finalize_scores_batched",
                    "optimize_constants_batched", "optimize_and_simplify_population_batched",
                    "reg_evol_cycle_batched", "reg_evol_cycle_lockstep", "s_r_cycle_lockstep")


def no_device():
    return srhip.device_count() == 0


def test_symbols_are_exported_with_the_headers_arities():
    protos = header_prototypes()
    lib = srhip.lib()
    for name, arity in GROUP_SYMBOLS.items():
        assert name in protos, f"{name} is not declared in include/srhip.h"
        ret, params = protos[name]
        assert ret == "int32_t" and len(params) == arity, (name, ret, params)
        assert hasattr(lib, name), f"libsrhip.so does not export {name}"
        assert len(_lib.SIGNATURES[name]) == arity, name
    declared = {n for n in protos if n.startswith("srhip_group_")}
    assert declared == set(GROUP_SYMBOLS), declared ^ set(GROUP_SYMBOLS)


@pytest.mark.parametrize("ndev", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("n", [0, 1, 2, 7, 8192, 8193, 10 ** 7])
def test_shard_range_equals_the_python_one_and_tiles(n, ndev):
    lib = srhip.lib()
    b, e = C.c_int64(-1), C.c_int64(-1)
    end = 0
    sizes = []
    for k in range(ndev):
        assert lib.srhip_group_shard_range(n, ndev, k, C.byref(b), C.byref(e)) == _lib.OK
        assert (b.value, e.value) == shard_range(n, k, ndev), (n, ndev, k)
        assert b.value == end and e.value >= b.value  # contiguous, in order; may be empty
        end = e.value
        sizes.append(e.value - b.value)
    assert end == n and max(sizes) - min(sizes) <= 1
    assert sizes == sorted(sizes, reverse=True) and sizes[: n % ndev] == [n // ndev + 1] * (n % ndev)


@pytest.mark.parametrize("n,ndev,k", [(10, 3, 3), (10, 3, -1), (10, 0, 0), (10, 17, 0), (10, -2, 0), (-1, 2, 0)])
def test_shard_range_rejects_out_of_range_arguments(n, ndev, k):
    b, e = C.c_int64(0), C.c_int64(0)
    assert srhip.lib().srhip_group_shard_range(n, ndev, k, C.byref(b), C.byref(e)) == _lib.ERR_INVALID
    assert srhip.lib().srhip_last_error()


def test_shard_range_null_outputs_are_invalid():
    assert srhip.lib().srhip_group_shard_range(10, 2, 0, None, None) == _lib.ERR_INVALID


def test_open_rejects_bad_member_lists():
    lib = srhip.lib()
    h = C.c_void_p()
    devs = (C.c_int32 * 17)()
    assert lib.srhip_group_open(devs, 0, C.byref(h)) == _lib.ERR_INVALID
    assert lib.srhip_group_open(devs, 17, C.byref(h)) == _lib.ERR_INVALID
    assert lib.srhip_group_open(None, 2, C.byref(h)) == _lib.ERR_INVALID
    assert lib.srhip_group_open(devs, 2, None) == _lib.ERR_INVALID
    neg = (C.c_int32 * 2)(0, -1)
    assert lib.srhip_group_open(neg, 2, C.byref(h)) == _lib.ERR_INVALID
    assert not h.value
    # null handles
    assert lib.srhip_group_close(None) == _lib.OK
    assert lib.srhip_group_info(None, None, None) == _lib.ERR_INVALID
    assert lib.srhip_group_ctx(None, 0, C.byref(h)) == _lib.ERR_INVALID
    assert lib.srhip_group_eval_loss(None, None, 0, None, None, None, None) == _lib.ERR_INVALID
    assert lib.srhip_group_eval_loss_grad(None, None, 0, None, None, None, None, None) == _lib.ERR_INVALID
    assert lib.srhip_group_program_set_constants(None, None) == _lib.ERR_INVALID
    assert lib.srhip_group_optimize_constants(None, None, None, None, None, None, None) == _lib.ERR_INVALID


def test_open_beyond_the_device_count_is_a_device_error():
    """A device index beyond srhip_device_count is SRHIP_ERR_DEVICE with a message, answered
    before any context is made: with no device visible every index is beyond the count."""
    lib = srhip.lib()
    h = C.c_void_p()
    beyond = srhip.device_count()  # 0 where no device is visible
    devs = (C.c_int32 * 2)(0, beyond)
    assert lib.srhip_group_open(devs, 2, C.byref(h)) == _lib.ERR_DEVICE
    assert lib.srhip_last_error().decode() and not h.value
    with pytest.raises(srhip.SrhipError) as e:
        srhip.DeviceGroup([beyond])
    assert e.value.code == _lib.ERR_DEVICE
    if no_device():
        assert "no HIP device" in str(e.value)


def test_python_classes_reject_bad_arguments():
    assert srhip.DeviceGroup and srhip.GroupDataset and srhip.GroupProgram
    for bad in ([], list(range(17)), [0, -1]):
        with pytest.raises(ValueError):
            srhip.DeviceGroup(bad)
    with pytest.raises(TypeError):
        srhip.DeviceGroup(3)
    o = srhip.Options(binary_operators=["+"], unary_operators=[])
    flat = srhip.flatten([srhip.Node(feature=1)], o, dtype=np.float32)
    with pytest.raises(TypeError):
        srhip.GroupProgram(None, flat, np.float32)
    with pytest.raises(TypeError):
        srhip.GroupDataset(None, np.zeros((1, 2), np.float32), np.zeros(2, np.float32))
    assert issubclass(srhip.GroupDataset, srhip.Dataset)
    from srhip.engine import group_shard_range

    assert group_shard_range(10, 3, 0) == (0, 4) and group_shard_range(2, 3, 2) == (2, 2)
    with pytest.raises(srhip.SrhipError):
        group_shard_range(10, 3, 3)


# ---- Julia, statically ----------------------------------------------------------------------
def test_group_ccalls_match_the_header():
    protos = header_prototypes()
    seen = set()
    for name, ret, argtypes, args in julia_ccalls():
        if not name.startswith("srhip_group_"):
            continue
        seen.add(name)
        cret, cparams = protos[name]
        assert ret == "Int32" and cret == "int32_t", name
        assert len(argtypes) == len(cparams) == len(args), name
        for jt, cp in zip(argtypes, cparams):
            assert _jl_kind(jt) == _c_kind(cp), f"{name}: Julia {jt} vs C {cp}"
    for need in ("srhip_group_open", "srhip_group_close", "srhip_group_ctx", "srhip_group_shard_range",
                 "srhip_group_dataset_create", "srhip_group_dataset_destroy", "srhip_group_program_create",
                 "srhip_group_program_destroy", "srhip_group_program_set_constants", "srhip_group_eval_loss",
                 "srhip_group_eval_loss_grad", "srhip_group_optimize_constants"):
        assert need in seen, need
    src = JL.read_text()
    assert re.search(r"mutable struct DeviceGroup\b", src)
    body = re.search(r"function group_dataset\(.*?\nend", src, re.S).group(0)
    assert "lock(CTX_LOCK) do" in body and "GROUP_DATASETS" in body and "finalizer(free!, d)" in body
    assert re.search(r"const GROUP_DATASETS = WeakKeyDict\{Dataset,", src)
    for sig in (r"function eval_loss_batch\([^)]*group::DeviceGroup\)", r"function eval_loss_grad\(p::GroupProgram",
                r"function optimize_constants_batch!\([^)]*group::DeviceGroup\)"):
        assert re.search(sig, src, re.S), sig


def _functions(code):
    """{name: body} of the top-level `function name(...) ... end` blocks."""
    return {m.group(1): m.group(0) for m in re.finditer(r"^function ([\w!]+)\(.*?^end", code, re.S | re.M)}


def _calls(body, name):
    """Argument strings of the calls of `name` in body (not its definitions)."""
    out = []
    for m in re.finditer(rf"(?<![\w.!]){re.escape(name)}\(", body):
        line_start = body.rfind("\n", 0, m.start()) + 1
        if body[line_start:m.start()].strip() in ("function", ""):
            continue  # `function name(` or a closure definition `name(...) = ...`
        depth, j = 0, m.end() - 1
        for j in range(m.end() - 1, len(body)):
            depth += body[j] == "("
            depth -= body[j] == ")"
            if depth == 0:
                break
        out.append(body[m.end():j])
    return out


def test_batched_callers_pass_the_device_down():
    code = "\n".join(ln.split("#")[0] for ln in BATCHED.read_text().splitlines())
    fns = _functions(code)
    for fn in DEVICE_FUNCTIONS:
        assert fn in fns, fn
        body = fns[fn]
        head = body[: body.index(" where {T}")]
        assert re.search(r"[;,]\s*(?:\w+::?[^;]*,\s*)*device::Int=0", head, re.S) and ";" in head, f"{fn}: no device keyword"
        # every SRHip call that runs on a device passes it on
        for call in ("eval_loss_batch", "eval_loss_batch_rowsets", "optimize_constants_batch!"):
            for args in _calls(body, "SRHip." + call):
                assert "device=device" in args, f"{fn}: SRHip.{call}({args})"
        # and so does every call of another of these functions: with the keyword, or through a
        # closure of the function that binds it
        for callee in DEVICE_FUNCTIONS:
            bound = re.search(rf"^\s*{callee}\([^)]*\) = BatchedCallers\.{callee}\([^)]*; device=device\)", body, re.M)
            for args in _calls(body, callee):
                assert bound or "device=device" in args, f"{fn}: {callee}({args})"
    used = set()
    for fn in DEVICE_FUNCTIONS:
        used |= {c for c in ("eval_loss_batch", "eval_loss_batch_rowsets", "optimize_constants_batch!")
                 if _calls(fns[fn], "SRHip." + c)}
    assert used == {"eval_loss_batch", "eval_loss_batch_rowsets", "optimize_constants_batch!"}
    # the helper that spreads the islands: member d gets the islands with (k - 1) % ndev == d
    helper = fns["s_r_cycle_devices"]
    assert "group::SRHip.DeviceGroup" in helper and "Threads.@spawn" in helper
    assert "collect(d:ndev:length(pops))" in helper and "device=Int(group.devices[d])" in helper
    assert "s_r_cycle_lockstep(" in helper
