"""Expression losses (include/srhip.h "expression losses") without a GPU: the ABI
surface, the registry and its error rules, the host statement of the semantics
(srhip_loss_expr_eval) against the oracle, the Python and Julia bindings.

The GPU side is tests/test_expr_loss_gpu.py; the expressions and the checker are
tests/expr_loss_cases.py.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import expr_loss_cases as E
import oracle
import srhip
from srhip import Node, _lib
from srhip import constants as K

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "srhip.h").read_text()
JL = (ROOT / "symbolicregression.jl_amd" / "julia" / "SRHip.jl").read_text()

# Host routines against the oracle: tests/test_precise_transcendentals.py asks for equal
# bits on all but at most 3 of its inputs (`bad.size <= 3`); the same here, per expression.
MAX_BIT_MISMATCHES = 3

NC, NF, NU, NB = K.NODE_CONST, K.NODE_FEATURE, K.NODE_UNARY, K.NODE_BINARY
ADD, SUB = K.BOP["ADD"], K.BOP["SUB"]


def create(kind, arg, consts=()):
    """(rc, handle) of srhip_loss_expr_create on a raw stream."""
    kind = np.asarray(kind, dtype=np.uint8)
    arg = np.asarray(arg, dtype=np.uint16)
    consts = np.asarray(consts, dtype=np.float64)
    out = C.c_int32(-1)
    rc = _lib.lib().srhip_loss_expr_create(kind.ctypes.data_as(C.POINTER(C.c_uint8)),
                                           arg.ctypes.data_as(C.POINTER(C.c_uint16)), len(kind),
                                           consts.ctypes.data_as(C.POINTER(C.c_double)), len(consts), C.byref(out))
    return rc, out.value


def test_header_declares_the_feature():
    for fn in ("srhip_loss_expr_create", "srhip_loss_expr_destroy", "srhip_loss_expr_eval"):
        assert re.search(rf"^int32_t {fn}\(", HEADER, re.M), fn
        assert hasattr(_lib.lib(), fn) and fn in _lib.SIGNATURES
    begin = int(re.search(r"#define SRHIP_EXPR_LOSS_BEGIN (\d+)", HEADER).group(1))
    assert begin == 1024 == K.EXPR_LOSS_BEGIN
    assert int(re.search(r"#define SRHIP_NUM_LOSSES (\d+)", HEADER).group(1)) == 22 == len(K.LOSSES)
    assert int(re.search(r"#define SRHIP_ABI_VERSION (\d+)", HEADER).group(1)) == 1 == _lib.lib().srhip_version()


def test_create_and_destroy_round_trip():
    L = _lib.lib()
    rc, h = create([NF, NF, NB], [0, 1, SUB])  # p - t
    assert rc == 0 and h >= K.EXPR_LOSS_BEGIN
    rc2, h2 = create([NF, NF, NB], [0, 1, SUB])
    assert rc2 == 0 and h2 > h  # handles are handed out once
    x = np.array([1.5, -2.0], dtype=np.float32)
    y = np.array([0.5, 3.0], dtype=np.float32)
    out = np.empty(2, dtype=np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.srhip_loss_expr_eval(h, K.F32, vp(x), vp(y), None, 2, vp(out)) == 0
    assert np.array_equal(out, x - y)
    assert L.srhip_loss_expr_destroy(h) == 0
    assert L.srhip_loss_expr_destroy(h) == _lib.ERR_INVALID  # gone
    assert L.srhip_loss_expr_eval(h, K.F32, vp(x), vp(y), None, 2, vp(out)) == _lib.ERR_INVALID
    assert L.srhip_loss_expr_eval(h2, K.F32, vp(x), vp(y), None, 2, vp(out)) == 0  # the other one lives
    assert L.srhip_loss_expr_destroy(h2) == 0


def test_error_cases():
    L = _lib.lib()
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    assert create([NF, NB], [0, ADD])[0] == INV                          # stack underflow
    assert create([NF, NU, NB], [0, 0, ADD])[0] == INV                   # underflow behind a unary
    assert create([NF, NF], [0, 1])[0] == INV                            # two values left
    assert create([NF, NF, NB], [0, 3, SUB])[0] == INV                   # feature index 3
    assert create([NF, NC, NB], [0, 0, ADD], [np.nan])[0] == INV         # a NaN constant
    assert create([NF, NC, NB], [0, 0, ADD], [np.inf])[0] == INV         # an infinite one
    assert create([NF, NC, NB], [0, 0, ADD], [])[0] == INV               # a constant leaf without its constant
    assert create([NF, 7, NB], [0, 0, ADD])[0] == INV                    # unknown node kind
    assert create([], [])[0] == INV                                      # empty
    # well formed, beyond the limits
    chain65 = [NF] + [NF, NB] * 32                                       # 65 nodes, stack depth 2
    assert create(chain65, [0] + [1, ADD] * 32)[0] == UNS
    chain63 = [NF] + [NF, NB] * 31                                       # 63 nodes: within the limits
    rc, h = create(chain63, [0] + [1, ADD] * 31)
    assert rc == 0 and L.srhip_loss_expr_destroy(h) == 0
    depth5 = [NF] * 5 + [NB] * 4                                         # 5 values live on the stack
    assert create(depth5, [0] * 5 + [ADD] * 4)[0] == UNS
    depth4 = [NF] * 4 + [NB] * 3
    rc, h = create(depth4, [0] * 4 + [ADD] * 3)
    assert rc == 0 and L.srhip_loss_expr_destroy(h) == 0
    assert create([NF, NU], [0, len(K.UOPS)])[0] == UNS                  # operator ids beyond the tables
    assert create([NF, NF, NB], [0, 1, len(K.BOPS)])[0] == UNS
    assert create([NF, NB], [0, len(K.BOPS)])[0] == INV                  # malformed wins over unsupported
    # kinds that are not registered
    x = np.zeros(1, dtype=np.float32)
    vp = x.ctypes.data_as(C.c_void_p)
    assert L.srhip_loss_expr_eval(K.EXPR_LOSS_BEGIN + 10**6, K.F32, vp, vp, None, 1, vp) == INV
    assert L.srhip_loss_expr_destroy(K.EXPR_LOSS_BEGIN + 10**6) == INV
    assert L.srhip_loss_expr_destroy(K.LOSS["L2"]) == INV
    # the tree compiler's testing hook has no code for these kinds
    o = srhip.Options(binary_operators=["+"], unary_operators=[])
    flat = srhip.flatten([o.make_binary("+", Node("x1"), Node("x2"))], o, dtype=np.float32)
    loss = E.expr_loss("SQ")
    with pytest.raises(srhip.Unsupported):
        srhip.engine.jit_compile(flat, loss=loss)


@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["E1", "E2", "E3", "E4", "E5"])
def test_value_matches_the_oracle(name, T):
    """ExprLoss.value (srhip_loss_expr_eval: the host routines of host_ops.h) on 1000 random
    (ŷ, y, w) against the oracle's evaluation of the same stream: the same rows are finite, E2
    (only exactly rounded operators) is bit-equal, the others bit-equal on all but at most 3 rows."""
    rng = np.random.default_rng(21)
    yhat = (3 * rng.standard_normal(1000)).astype(T)
    y = (3 * rng.standard_normal(1000)).astype(T)
    y[:5] = yhat[:5]  # r = 0
    y[5] = 0
    w = np.abs(rng.standard_normal(1000)).astype(T)
    loss = E.expr_loss(name)
    got = loss.value(yhat, y, w)
    assert got.dtype == T and got.shape == yhat.shape
    # the oracle row by row: a row alone fails iff a value of its loss expression is non-finite
    k, a, c = E.loss_stream(name)
    ref = np.full(1000, np.nan, dtype=T)
    with np.errstate(all="ignore"):
        for i in range(1000):
            out, fin = oracle.eval_tree(k, a, c, np.array([[yhat[i]], [y[i]], [w[i]]], dtype=T), dtype=T)
            if fin:
                ref[i] = out[0]
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (name, np.flatnonzero(np.isfinite(got) != fin)[:10])
    if name == "E5":
        assert 0 < fin.sum() < 1000  # log(p / t) is NaN where the signs differ
    else:
        assert fin.all()
    bits = np.int32 if T == np.float32 else np.int64
    bad = np.flatnonzero(got[fin].view(bits) != ref[fin].view(bits))
    assert bad.size <= (0 if name == "E2" else MAX_BIT_MISMATCHES), (name, bad[:5], got[fin][bad[:5]], ref[fin][bad[:5]])
    if name != "E3":  # w unused: the two-argument form gives the same values
        assert np.array_equal(loss.value(yhat, y), got, equal_nan=True)
    else:
        with pytest.raises(srhip.SrhipError) as e:
            loss.value(yhat, y)
        assert e.value.code == _lib.ERR_INVALID


def test_problem_a_counts():
    """The counts the GPU tests rely on, from the oracle alone: 197 of the 200 trees succeed at
    n = 1, 513 and 3000 in both dtypes; E1-E4 are finite on all of them; E5 on 83 at n = 1 and
    on none at n >= 513."""
    for T in (np.float32, np.float64):
        for n in (1, 513, 3000):
            o, trees, flat, X, y, w, yhat, ok = E.problem(T, n)
            assert int(ok.sum()) == 197, (T, n)
            for name in ("E1", "E2", "E3", "E4", "E5"):
                ref, _ = E.reference_sums(name, yhat, y, w, ok, T)
                nfin = int(np.isfinite(ref[ok]).sum())
                want = 197 if name != "E5" else (83 if n == 1 else 0)
                assert nfin == want, (np.dtype(T).name, n, name, nfin)


def test_options_keep_the_object():
    lo = E.loss_options()
    loss = srhip.ExprLoss(E.e1(lo), lo)
    o = srhip.Options(binary_operators=["+", "-"], unary_operators=[], elementwise_loss=loss)
    assert o.elementwise_loss is loss
    k = loss.kind
    assert k >= K.EXPR_LOSS_BEGIN and loss.kind == k and o.elementwise_loss.kind == k
    assert loss.params is None and loss.param == 0.0 and not loss.uses_weights
    assert srhip.ExprLoss(E.e3(lo), lo).uses_weights
    other = srhip.ExprLoss(E.e1(lo), lo)
    assert other.kind != k
    # finalisation destroys the handle
    del other
    loss.destroy()
    x = np.ones(1, dtype=np.float32)
    vp = x.ctypes.data_as(C.c_void_p)
    assert _lib.lib().srhip_loss_expr_eval(k, K.F32, vp, vp, None, 1, vp) == _lib.ERR_INVALID
    # an operator outside the engine's table cannot be flattened
    bad = srhip.Options(binary_operators=["+"], unary_operators=["asin"])
    with pytest.raises(srhip.Unsupported):
        srhip.ExprLoss(bad.make_unary("asin", Node("x1")), bad)
    # beyond the limits: Unsupported, so a caller can fall back
    deep = Node("x1")
    for _ in range(4):
        deep = lo.make_binary("+", Node("x1"), deep)  # x1 x1 x1 x1 x1 + + + +: 5 live values
    with pytest.raises(srhip.Unsupported):
        srhip.ExprLoss(deep, lo)


def test_julia_binding_defines_the_expression_loss():
    assert re.search(r"^(mutable )?struct ExprLoss\b.*<: Function", JL, re.M)
    assert re.search(r"^loss_code\(l::ExprLoss\) = \(l\.kind, 0\.0\)", JL, re.M)
    assert re.search(r"^const SRHIP_EXPR_LOSS_BEGIN = Int32\(1024\)", JL, re.M)
    assert re.search(r"^function \(l::ExprLoss[^)]*\)\(x, y, w=", JL, re.M)  # callable with 2 and 3 arguments
    from test_julia_binding import header_prototypes, julia_ccalls

    protos = header_prototypes()
    calls = {name: argtypes for name, _, argtypes, _ in julia_ccalls()}
    for fn in ("srhip_loss_expr_create", "srhip_loss_expr_destroy"):
        assert fn in calls, fn
        assert len(calls[fn]) == len(protos[fn][1]), (fn, calls[fn], protos[fn][1])
