"""Expression operators (include/srhip.h "expression operators") without a GPU: the ABI
surface, the registry and its error rules, the host statement of the semantics (srhip_op_eval on
a handle) against the oracle's own operators, the constant map of the expanded programs, the
tree compiler's hooks, the Python and Julia bindings.

The GPU side is tests/test_expr_ops_gpu.py; the operators and the expansion are
tests/expr_op_cases.py.
"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import expr_op_cases as E
import oracle
import srhip
from srhip import Node, _lib
from srhip import constants as K
from srhip.engine import debug_constant_map, jit_compile
from test_jit import LLVM

ROOT = Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "srhip.h").read_text()
JL = (ROOT / "symbolicregression.jl_amd" / "julia" / "SRHip.jl").read_text()

NC, NF, NU, NB = K.NODE_CONST, K.NODE_FEATURE, K.NODE_UNARY, K.NODE_BINARY
ADD, MUL = K.BOP["ADD"], K.BOP["MUL"]
COS = K.UOP["COS"]
INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]


def create(arity, kind, arg, consts=()):
    """(rc, handle) of srhip_op_expr_create on a raw stream."""
    kind = np.asarray(kind, dtype=np.uint8)
    arg = np.asarray(arg, dtype=np.uint16)
    consts = np.asarray(consts, dtype=np.float64)
    out = C.c_int32(-1)
    rc = _lib.lib().srhip_op_expr_create(arity, kind.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         arg.ctypes.data_as(C.POINTER(C.c_uint16)), len(kind),
                                         consts.ctypes.data_as(C.POINTER(C.c_double)), len(consts), C.byref(out))
    return rc, out.value


def op_eval(T, arity, op_id, a, b=0.0):
    out = C.c_double(0.0)
    rc = _lib.lib().srhip_op_eval(K.F32 if T == np.float32 else K.F64, arity, op_id, float(a), float(b), C.byref(out))
    return rc, out.value


def raw_flat(kind, arg, consts=(), T=np.float32):
    """One tree as a FlatTrees from a raw stream."""
    from srhip.node import FlatTrees

    return FlatTrees(np.array([0, len(kind)], dtype=np.int32), np.asarray(kind, dtype=np.uint8),
                     np.asarray(arg, dtype=np.uint16), np.array([0, len(consts)], dtype=np.int32),
                     np.asarray(consts, dtype=T), np.array([len(kind)], dtype=np.int64))


def compile_rc(flat, T=np.float32):
    """Status of a host compile of `flat` (the constant-map hook compiles the trees first)."""
    try:
        debug_constant_map(flat, flat.consts, T)
    except srhip.SrhipError as e:
        return e.code
    return 0


def test_header_declares_the_feature():
    for fn in ("srhip_op_expr_create", "srhip_op_expr_destroy"):
        assert re.search(rf"^int32_t {fn}\(", HEADER, re.M), fn
        assert hasattr(_lib.lib(), fn) and fn in _lib.SIGNATURES
    begin = int(re.search(r"#define SRHIP_EXPR_OP_BEGIN (\d+)", HEADER).group(1))
    assert begin == 1024 == K.EXPR_OP_BEGIN
    assert int(re.search(r"#define SRHIP_ABI_VERSION (\d+)", HEADER).group(1)) == 1 == _lib.lib().srhip_version()


def test_registry_round_trip():
    L = _lib.lib()
    rc, h = create(1, [NF, NU], [0, COS])
    assert rc == 0 and h >= K.EXPR_OP_BEGIN
    rc2, h2 = create(1, [NF, NU], [0, COS])
    assert rc2 == 0 and h2 > h  # handles are handed out once
    assert op_eval(np.float64, 1, h, 0.5) == (0, float(oracle.unop(COS, np.float64(0.5), dtype=np.float64)))
    assert op_eval(np.float64, 2, h, 0.5)[0] == INV  # the wrong arity
    assert L.srhip_op_expr_destroy(h) == 0
    assert L.srhip_op_expr_destroy(h) == INV  # gone
    assert op_eval(np.float64, 1, h, 0.5)[0] == INV
    assert op_eval(np.float64, 1, h2, 0.5)[0] == 0  # the other one lives
    rc3, h3 = create(1, [NF, NU], [0, COS])
    assert rc3 == 0 and h3 > h2  # a destroyed handle is not reused
    assert L.srhip_op_expr_destroy(h2) == 0 and L.srhip_op_expr_destroy(h3) == 0
    assert L.srhip_op_expr_destroy(h3 + 10**4) == INV and L.srhip_op_expr_destroy(COS) == INV


def test_error_cases():
    L = _lib.lib()
    assert create(1, [NF, NB], [0, ADD])[0] == INV                          # stack underflow
    assert create(2, [NF, NF], [0, 1])[0] == INV                            # two values left
    assert create(1, [NF, NF, NB], [0, 1, ADD])[0] == INV                   # feature index beyond the arity
    assert create(2, [NF, NF, NB], [0, 2, ADD])[0] == INV
    assert create(3, [NF], [0])[0] == INV and create(0, [NF], [0])[0] == INV  # the arity itself
    assert create(1, [NF, NC, NB], [0, 0, ADD], [np.nan])[0] == INV         # a NaN constant
    assert create(1, [NF, NC, NB], [0, 0, ADD], [np.inf])[0] == INV         # an infinite one
    assert create(1, [NF, NC, NB], [0, 0, ADD], [])[0] == INV               # a constant leaf without its constant
    assert create(1, [NF, 7, NB], [0, 0, ADD])[0] == INV                    # unknown node kind
    assert create(1, [], [])[0] == INV                                      # empty
    # well formed, beyond the limits
    assert create(1, [NF] + [NF, NB] * 32, [0] + [0, ADD] * 32)[0] == UNS   # 65 nodes
    rc, h = create(1, [NF] + [NF, NB] * 31, [0] + [0, ADD] * 31)            # 63 nodes
    assert rc == 0 and L.srhip_op_expr_destroy(h) == 0
    assert create(1, [NF] * 5 + [NB] * 4, [0] * 5 + [ADD] * 4)[0] == UNS    # 5 values live on the stack
    rc, h = create(1, [NF] * 4 + [NB] * 3, [0] * 4 + [ADD] * 3)
    assert rc == 0 and L.srhip_op_expr_destroy(h) == 0
    assert create(1, [NF, NU], [0, len(K.UOPS)])[0] == UNS                  # operator ids beyond the tables
    assert create(2, [NF, NF, NB], [0, 1, len(K.BOPS)])[0] == UNS
    inner = E.expr_op("custom_cos").op_id
    assert create(1, [NF, NU], [0, inner])[0] == UNS                        # no expression operator inside a body
    assert create(1, [NF, NB], [0, len(K.BOPS)])[0] == INV                  # malformed wins over unsupported


def test_tree_error_cases():
    """Handles inside trees: unknown ids are unsupported, a destroyed handle and a handle of the
    wrong arity are invalid."""
    u = E.expr_op("custom_cos").op_id
    b = E.expr_op("my_func_a").op_id
    assert compile_rc(raw_flat([NF, NU], [0, u])) == 0
    assert compile_rc(raw_flat([NF, NF, NB], [0, 1, b])) == 0
    assert compile_rc(raw_flat([NF, NU], [0, b])) == INV           # a binary operator in a unary node
    assert compile_rc(raw_flat([NF, NF, NB], [0, 1, u])) == INV
    assert compile_rc(raw_flat([NF, NU], [0, len(K.UOPS)])) == UNS  # between the table and the handles
    assert compile_rc(raw_flat([NF, NU], [0, 60000])) == UNS        # never handed out
    rc, h = create(1, [NF, NU], [0, COS])
    assert rc == 0 and compile_rc(raw_flat([NF, NU], [0, h])) == 0
    assert _lib.lib().srhip_op_expr_destroy(h) == 0
    assert compile_rc(raw_flat([NF, NU], [0, h])) == INV            # destroyed


def compose(name, a, b, T):
    """The definition `name` at the scalars (a, b), composed from oracle.unop / oracle.binop in T."""
    U, B = K.UOP, K.BOP
    un = lambda op, x: T(oracle.unop(U[op], x, dtype=T))
    bi = lambda op, x, y: T(oracle.binop(B[op], x, y, dtype=T))
    c = T  # a body constant, rounded to T once
    if name == "custom_cos":
        return un("SQUARE", un("COS", a))
    if name == "op3":
        return bi("ADD", un("SIN", a), un("COS", a))
    if name == "my_func_a":
        return bi("MUL", un("SQUARE", a), b)
    if name == "my_func_c":
        return bi("ADD", bi("MUL", a, b), c(0.3))
    if name == "nexp":
        return un("INV", un("EXP", a))
    if name == "op2":
        return bi("ADD", un("SQUARE", a), un("INV", bi("ADD", un("SQUARE", b), c(0.1))))
    if name == "dbl":
        return bi("ADD", bi("MUL", a, a), a)
    return un("LOG", a)


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("name", sorted(E.DEFS))
def test_op_eval_equals_the_composition_of_the_oracle(name, T):
    """srhip_op_eval on a handle against the composition of oracle.unop / oracle.binop, bit for
    bit: 400 normal draws, and arguments where the body overflows inside (exp at 100 / 1000),
    is NaN (log of a negative) or gets a non-finite argument."""
    rng = np.random.default_rng(5)
    a = np.concatenate([3 * rng.standard_normal(400), [0.0, -0.0, 100.0, 1000.0, -1000.0, np.inf, -np.inf, np.nan, -2.0]]).astype(T)
    b = np.concatenate([3 * rng.standard_normal(400), [0.0, 1.0, -1.0, 0.5, 2.0, 1.0, np.inf, 1.0, np.nan]]).astype(T)
    op = E.expr_op(name)
    with np.errstate(all="ignore"):
        ref = np.array([compose(name, x, y, T) for x, y in zip(a, b)], dtype=T)
    got = np.array([op_eval(T, op.arity, op.op_id, x, y)[1] for x, y in zip(a, b)]).astype(T)
    bits = np.int32 if T == np.float32 else np.int64
    same = (got.view(bits) == ref.view(bits)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), (name, a[~same][:5], got[~same][:5], ref[~same][:5])
    if name == "nexp":  # the opaque case: exp overflows, the operator's value is 0
        big = T(100.0 if T == np.float32 else 1000.0)
        assert op_eval(T, 1, op.op_id, big) == (0, 0.0)


def cmap_trees():
    """Hand-built trees for the constant map: constants as arguments used twice in a body,
    feature-free subtrees that hold an operator, body constants next to tree constants."""
    o = E.options(E.NONLOSSY + E.LOSSY)
    x1, x2, c = (lambda: Node("x1")), (lambda: Node("x2")), (lambda v: Node(val=v))
    U, B = o.make_unary, o.make_binary
    return o, [
        U("dbl", c(1.5)),                                       # folds: the operator in a feature-free subtree
        B("+", x1(), U("dbl", c(1.5))),
        U("dbl", B("*", c(0.7), x1())),                          # a computed argument in a slot, used three times
        B("op2", x1(), c(0.9)),                                  # a constant argument used once, next to a body constant
        B("op2", c(0.4), x2()),
        B("my_func_c", c(1.1), x1()),
        B("my_func_c", B("+", x1(), c(2.0)), B("*", c(0.5), x2())),
        U("op3", c(0.3)),                                        # folds
        B("*", U("op3", B("+", c(0.3), c(0.2))), x1()),           # a folded argument subtree
        B("my_func_a", U("custom_cos", c(2.0)), B("-", x2(), c(1.0))),
        U("nexp", B("my_func_a", c(1.2), c(0.8))),               # operator inside operator, all feature-free
        B("+", U("nexp", B("my_func_a", c(1.2), x1())), c(3.0)),
        B("my_func_a", c(2.5), c(2.5)),
        U("cos", B("op2", c(0.1), c(0.2))),
    ]


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("grad", [False, True], ids=["loss", "grad"])
@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep_layout"])
def test_constant_map(T, grad, keep):
    """srhip_debug_constant_map: new constants written through the map give the programs of a
    fresh compile (out_mismatch == 0, no relayout), for loss and gradient programs, on the
    hand-built trees and on 200 random trees over the non-lossy and the lossy operators."""
    o, trees = cmap_trees()
    rnd = list(srhip.random_population(200, o, 3, T, seed=3, maxsize=15))
    flat = srhip.flatten(trees + rnd, o, dtype=T)
    rng = np.random.default_rng(8)
    new = (flat.consts * (1 + 0.5 * rng.standard_normal(len(flat.consts)))).astype(T)
    mm, rc, rl = debug_constant_map(flat, new, T, grad=grad, keep_layout=keep)
    assert (mm, rl) == (0, 0), (mm, rc, rl)
    # a constant that makes a folded operator's output non-finite: the verdict follows
    new2 = new.copy()
    new2[0] = np.inf
    mm, rc, rl = debug_constant_map(flat, new2, T, grad=grad, keep_layout=keep)
    assert mm == 0, (mm, rc, rl)


def test_slot_overflow_is_unsupported():
    """The operator's two computed arguments sit in reserved slots, the second evaluated above the
    first: my_func_a(d15, d15), d15 a balanced tree that needs 15 slots, needs 16 and compiles; the
    sum of two of them needs 17: UNSUPPORTED with the existing message. (Children are shared
    objects: the flattener writes them out once per reference.)"""
    o = E.options(("my_func_a",))
    d = o.make_unary("cos", Node("x1"))
    for _ in range(15):
        d = o.make_binary("+", d, d)
    f = o.make_binary("my_func_a", d, d)
    assert compile_rc(srhip.flatten([f], o, dtype=np.float32)) == 0
    flat = srhip.flatten([o.make_binary("+", f, f)], o, dtype=np.float32)
    for grad in (False, True):
        with pytest.raises(srhip.Unsupported, match="more than 16 stack slots"):
            debug_constant_map(flat, flat.consts, np.float32, grad=grad)


@pytest.mark.skipif(not (LLVM / "llvm-mc").exists(), reason="llvm-mc not installed")  # as tests/test_jit.py
def test_jit_hooks_skip_operator_trees():
    """srhip_jit_compile and srhip_jit_compile_grad, Float32 and Float64: a tree that holds an
    expression operator is left out of out_offsets, its neighbours are compiled."""
    o = E.options(("custom_cos", "my_func_c"))
    x1, x2 = Node("x1"), Node("x2")
    trees = [o.make_binary("+", x1, Node(val=1.5)),
             o.make_unary("custom_cos", o.make_binary("*", Node(val=2.0), x2)),
             o.make_binary("my_func_c", x1, Node(val=0.5)),
             o.make_unary("cos", o.make_binary("*", x1, Node(val=0.7)))]
    for T in (np.float32, np.float64):
        flat = srhip.flatten(trees, o, dtype=T)
        for kw in (dict(), dict(grad=True)):
            _, _, offs = jit_compile(flat, **kw)
            assert set(offs) == {0, 3}, (T, kw, offs)


def test_options_and_flatten_give_the_handle():
    o = E.options(("custom_cos", "my_func_a"))
    cc, fa = E.expr_op("custom_cos"), E.expr_op("my_func_a")
    assert o.unary_operators == ("cos", "exp", "custom_cos") and o.binary_operators == ("+", "-", "*", "/", "my_func_a")
    b, u = o.engine_operator_ids()
    assert u == [K.UOP["COS"], K.UOP["EXP"], cc.op_id] and b[-1] == fa.op_id and cc.op_id >= K.EXPR_OP_BEGIN
    t = o.make_binary("my_func_a", o.make_unary("custom_cos", Node("x1")), Node(val=2.0))
    flat = srhip.flatten([t], o, dtype=np.float32)
    assert flat.kind.tolist() == [NF, NU, NC, NB] and flat.arg.tolist() == [0, cc.op_id, 0, fa.op_id]
    assert srhip.string_tree(t, o) == "my_func_a(custom_cos(x1), 2.0)"
    # the wrong list for its arity
    bad = srhip.Options(binary_operators=["+", cc], unary_operators=["cos"])
    with pytest.raises(srhip.Unsupported):
        bad.engine_operator_ids()
    # an unknown name still has no id
    with pytest.raises(srhip.Unsupported):
        srhip.Options(binary_operators=["+"], unary_operators=["custom_cos"]).engine_operator_ids()
    # the host folding of the search mirror evaluates the operator through its handle
    from srhip.evolution import _op_eval

    assert _op_eval(np.float64, 1, cc.op_id, 0.5) == float(np.cos(0.5)) ** 2 or \
        abs(_op_eval(np.float64, 1, cc.op_id, 0.5) - np.cos(0.5) ** 2) < 1e-15
    # finalisation destroys the handle
    tmp = srhip.ExprOp("tmp_op", E.dbl(E.prim_options()), E.prim_options(), 1)
    h = tmp.op_id
    assert op_eval(np.float64, 1, h, 2.0) == (0, 6.0)
    del tmp
    import gc

    gc.collect()
    assert op_eval(np.float64, 1, h, 2.0)[0] == INV
    # beyond the limits: Unsupported, so a caller can fall back
    po = E.prim_options()
    deep = Node("x1")
    for _ in range(4):
        deep = po.make_binary("+", Node("x1"), deep)  # 5 live values
    with pytest.raises(srhip.Unsupported):
        srhip.ExprOp("deep", deep, po, 1)


def test_julia_binding_registers_operators():
    assert re.search(r"^function register_operator!\(f, tree::Node\{T\}, operators; arity", JL, re.M)
    assert re.search(r"^const SRHIP_EXPR_OP_BEGIN = Int32\(1024\)", JL, re.M)
    # op_id asks the registry before srhip_op_lookup
    body = JL[JL.index("function op_id(op, arity)"):]
    body = body[:body.index("\nend\n")]
    assert body.index("EXPR_OPS") < body.index("srhip_op_lookup")
    from test_julia_binding import header_prototypes, julia_ccalls

    protos = header_prototypes()
    calls = {name: argtypes for name, _, argtypes, _ in julia_ccalls()}
    for fn in ("srhip_op_expr_create", "srhip_op_expr_destroy"):
        assert fn in calls, fn
        assert len(calls[fn]) == len(protos[fn][1]), (fn, calls[fn], protos[fn][1])
