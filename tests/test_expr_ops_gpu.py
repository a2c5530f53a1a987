"""Expression operators on the GPU: a custom operator written as an engine tree, expanded on
the host into the enclosing tree's program and run by the 16-slot interpreter kernels of the
OPSET_EXPR operator set (slot reads, the argument check, the no-mark flag of body instructions).

The oracle has no custom operators: the checker is the oracle on the EXPANDED tree
(tests/expr_op_cases.py `expand`). For bodies of non-lossy operators expansion cannot change
did_succeed, so values and verdicts of an operator tree and of its expansion are the same; for
lossy bodies the tests state the difference (nothing inside a body is checked).

Bounds: loss sums by check_sums / RTOL of tests/test_margin_losses_gpu.py; gradients by the bar
of test_gradients_match_the_reference of tests/test_expr_loss_gpu.py (rtol·Σ|terms| plus what a
4-ulp move of r = ŷ - y does to the L2 seed 2r); per-row values bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine opens the device: the process then holds one HIP runtime)

import expr_loss_cases as EL
import expr_op_cases as E
import oracle
import srhip
from srhip import Node, _lib
from srhip import constants as K
from test_margin_losses_gpu import RTOL, check_sums, program

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
L2, L1 = K.LOSS["L2"], K.LOSS["L1"]

# Problem B (tests/expr_op_cases.py problem, seed 7, 250 trees, features 8·N(0,1)), from the
# oracle alone on the expanded trees: (succeeding, failing) trees per n.
ORACLE_COUNTS = {
    np.float32: {1: (238, 12), 256: (227, 23), 513: (227, 23), 3000: (224, 26)},
    np.float64: {1: (242, 8), 256: (233, 17), 513: (233, 17), 3000: (230, 20)},
}
# of the succeeding ones, those whose L2 sum is well conditioned by the oracle's own spread (oracle_b)
ORACLE_CONDITIONED = {
    np.float32: {1: 132, 256: 169, 513: 169, 3000: 166},
    np.float64: {1: 238, 256: 222, 513: 221, 3000: 219},
}


def bits(a):
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


@functools.lru_cache(maxsize=None)
def oracle_b(T, n):
    """The oracle on the expanded trees of problem B: (ŷ, ok, Σ r², ok of the L2 call, and which
    sums are well conditioned). The wide features that make trees fail also feed exp-sized values
    to cos, where a one-ulp difference in a transcendental moves the result without limit: no
    bound relative to Σ|ℓ| holds for such a tree. The oracle alone decides which trees those are
    (tests/numerics.py: the spread of its own sums under 4-ulp perturbations and 4-ulp noise on
    every transcendental value): a sum is compared when 4 · spread is within the bound."""
    from numerics import loss_spread_flat

    o, trees, flat, xflat, X, y, w = E.problem(T, n)
    with np.errstate(all="ignore"):
        yhat, ok = oracle.eval_trees(xflat, X, dtype=T)
        sums, _, lok = oracle.eval_loss_batch(xflat, X, y, dtype=T)
        spread = loss_spread_flat(xflat, X, y, None, T, srhip.L2DistLoss())
        cond = lok & np.isfinite(sums) & (4 * spread <= RTOL[np.dtype(T)] * np.abs(sums) + 4 * float(np.finfo(T).eps) * n)
    for a in (yhat, ok, sums, lok, cond):
        a.setflags(write=False)
    return yhat, ok, sums, lok, cond


def op_eval(T, op, a, b=0.0):
    out = C.c_double(0.0)
    assert _lib.lib().srhip_op_eval(K.F32 if T == np.float32 else K.F64, op.arity, op.op_id, float(a), float(b),
                                    C.byref(out)) == 0
    return T(out.value)


@pytest.mark.parametrize("T", DTYPES)
@pytest.mark.parametrize("n", [1, 256, 513, 3000])
def test_operator_trees_equal_their_expansions(gpu_ctx, n, T):
    """Check 1. 250 random trees over {+, -, *, /, cos, exp} and the non-lossy operators (216 of
    them hold an operator), against their expansions run interpreted: per-row values and
    did_succeed bit-identical; the L2 sums against the oracle on the expansions within the
    bound, on the trees whose sum the oracle itself shows well conditioned (oracle_b). The oracle alone finds at least half of the trees succeeding and at least five
    failing at every n (ORACLE_COUNTS)."""
    o, trees, flat, xflat, X, y, w = E.problem(T, n)
    yhat, rok, rsum, lok, cond = oracle_b(T, n)
    assert (int(rok.sum()), int((~rok).sum())) == ORACLE_COUNTS[T][n]
    assert int(cond.sum()) == ORACLE_CONDITIONED[T][n] >= flat.ntrees // 2
    assert rok.sum() >= flat.ntrees // 2 and (~rok).sum() >= 5 and np.array_equal(rok, lok)
    is_op = (flat.kind >= K.NODE_UNARY) & (flat.arg >= K.EXPR_OP_BEGIN)
    assert sum(bool(is_op[flat.node_off[t]:flat.node_off[t + 1]].any()) for t in range(flat.ntrees)) == 216
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = program(ctx, flat, T, "0")
    xprog = program(ctx, xflat, T, "0")
    nt, tot, nodes = prog.info()
    assert np.array_equal(nodes, flat.nodes) and tot == int(flat.nodes.sum())  # one node per operator
    out, ok = prog.eval_tree_array(ds)
    xout, xok = xprog.eval_tree_array(ds)
    assert ctx.last_tree_code() == 0
    assert np.array_equal(ok, xok) and np.array_equal(ok, rok)
    assert np.array_equal(bits(out[ok]), bits(xout[ok]))
    s, wsum, lk = prog.eval_loss(ds, L2)
    assert np.array_equal(np.asarray(lk).astype(bool), rok) and wsum == float(n)
    # (a sum the oracle overflows to +Inf is matched exactly; the well-conditioned finite ones meet the bound)
    nfin = check_sums(s, rsum, np.abs(rsum), float(n), rok & (cond | ~np.isfinite(rsum)), T,
                      f"L2 {np.dtype(T).name} n={n}")
    assert nfin == int(cond.sum())
    assert np.isnan(s[~rok]).all()


@pytest.mark.parametrize("T", DTYPES)
def test_opaque_semantics(gpu_ctx, T):
    """Check 2. Row 7 has x1 = 100 (Float32) / 1000 (Float64), where exp overflows.
    nexp(x1) + x2 succeeds and equals x2 there (inv(Inf) = 0 inside the body is not checked); its
    expansion fails. nexp(exp(x1)) fails: the argument is checked. ulog on a negative argument
    gives NaN: the result fails the tree. Values equal srhip_op_eval bit for bit: at the rows with
    x1 = 100 / 1000 in both dtypes, and on the 512 other rows in Float32, whose device and host
    transcendentals are the same arithmetic. The Float64 device routines are not the host's libm:
    on those rows Float64 values stay within the engine's per-operator bar of 4 ulp per
    transcendental (tests/numerics.py), two of them in a body."""
    o = E.options(("nexp", "ulog"))
    po = E.prim_options()
    nexp, ulog = E.expr_op("nexp"), E.expr_op("ulog")
    U, B = o.make_unary, o.make_binary
    trees = [B("+", U("nexp", Node("x1")), Node("x2")),
             U("nexp", U("exp", Node("x1"))),
             U("ulog", Node("x1")),
             U("ulog", B("*", Node("x2"), Node("x2"))),
             U("exp", U("nexp", Node("x1")))]  # a lossy consumer marks the operator's result, not its inside
    big = T(100.0 if T == np.float32 else 1000.0)
    for n in (1, 513):
        X = np.random.default_rng(31).standard_normal((2, n)).astype(T)
        X[1] = np.abs(X[1]) + T(0.5)
        row = 7 if n > 7 else 0
        X[0, row] = big
        if n > 1:
            X[0, 3] = T(-2.0)
        y = np.zeros(n, dtype=T)
        flat = srhip.flatten(trees, o, dtype=T)
        xflat = srhip.flatten([E.expand(t, o) for t in trees], po, dtype=T)
        ctx = gpu_ctx
        ds = srhip.DeviceDataset(ctx, X, y)
        out, ok = srhip.Program(ctx, flat, T).eval_tree_array(ds)
        xout, xok = srhip.Program(ctx, xflat, T).eval_tree_array(ds)
        with np.errstate(all="ignore"):
            _, rok = oracle.eval_trees(xflat, X, dtype=T)
        assert np.array_equal(xok, rok)
        neg = bool((X[0] < 0).any())
        assert ok.tolist() == [True, False, not neg, True, True], (n, ok)
        assert xok.tolist() == [False, False, not neg, True, False], (n, xok)
        want0 = np.array([op_eval(T, nexp, v) for v in X[0]], dtype=T) + X[1]
        want3 = np.array([op_eval(T, ulog, v) for v in X[1] * X[1]], dtype=T)
        want4 = np.array([oracle.unop(K.UOP["EXP"], op_eval(T, nexp, v), dtype=T) for v in X[0]], dtype=T)
        assert op_eval(T, nexp, big) == 0 and out[0, row] == X[1, row] and out[4, row] == T(1.0)
        assert bits(out[0])[row] == bits(want0)[row] and bits(out[4])[row] == bits(want4)[row]
        for got, want, nops in ((out[0], want0, 2), (out[3], want3, 1), (out[4], want4, 3)):
            if T == np.float32:
                assert np.array_equal(bits(got), bits(want))
            else:
                assert np.all(np.abs(got - want) <= 4 * nops * np.spacing(np.abs(want)))
        # the loss entry agrees with the per-row one
        _, _, lok = srhip.Program(ctx, flat, T).eval_loss(ds, L2)
        assert np.array_equal(np.asarray(lok).astype(bool), ok)


def grad_trees(o):
    x1, x2, c = (lambda: Node("x1")), (lambda: Node("x2")), (lambda v: Node(val=v))
    U, B = o.make_unary, o.make_binary
    return [
        U("dbl", B("*", c(0.7), x1())),                          # the tangent passes through a slot and three uses
        B("op2", x1(), c(0.9)),                                  # a constant argument; a body constant next to it
        B("op2", c(0.4), x2()),
        B("my_func_c", c(1.1), x1()),                            # body constant 0.3 next to a tree constant
        B("my_func_c", B("+", x1(), c(2.0)), B("*", c(0.5), x2())),
        B("my_func_a", U("custom_cos", B("*", c(2.0), x1())), B("-", x2(), c(1.0))),
        B("+", U("op3", B("+", c(0.3), c(0.2))), B("*", c(1.5), x1())),  # a feature-free argument (no folding here)
        U("dbl", c(1.5)),                                        # a constant argument used three times
        B("*", U("dbl", B("my_func_c", c(0.6), x2())), c(0.25)),  # operator inside an operator's argument
        U("cos", B("op2", B("*", c(0.1), x1()), B("*", c(0.2), x2()))),
        B("+", B("+", B("*", c(0.1), x1()), B("*", c(0.2), x2())),   # six constants: two tangent groups
          U("dbl", B("+", B("*", c(0.3), x1()), B("+", B("*", c(0.4), x2()), B("*", c(0.5), c(0.6)))))),
    ]


@pytest.mark.parametrize("T", DTYPES)
def test_gradients_match_the_reference(gpu_ctx, T):
    """Check 3. srhip_eval_loss_grad (L2) on hand-built trees and on 150 random trees over the
    non-lossy operators, dbl and op2, against oracle.eval_grad_consts on the expanded tree: a
    constant that the expansion duplicates is compared with the sum of its copies, a body constant
    has no gradient. Bound per constant: rtol·Σ|terms| plus what a 4-ulp move of r does to the
    seed 2r (the bar of tests/test_expr_loss_gpu.py). Trees that the oracle fails on their
    expansion are left out (an operator tree may succeed where its expansion fails), and so are
    the random trees whose L2 sum the oracle itself shows ill conditioned (as oracle_b: cos of an
    exp-sized value moves by more than the bound under one ulp of noise; 24 of 130 Float32 and 2
    of 131 Float64 trees with constants)."""
    from numerics import loss_spread_flat

    names = E.NONLOSSY + ("dbl", "op2")
    o = E.options(names)
    n = 513
    rnd = list(srhip.random_population(150, o, 2, T, seed=21, maxsize=15))
    trees = grad_trees(o) + rnd
    nhand = len(trees) - len(rnd)
    flat = srhip.flatten(trees, o, dtype=T)
    X = np.random.default_rng(41).standard_normal((2, n)).astype(T)
    y = (np.cos(X[0]) + X[1]).astype(T)
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = srhip.Program(ctx, flat, T)
    s, g, wsum, ok = prog.eval_loss_grad(ds, L2)
    assert ctx.last_tree_code() == 0
    info = prog.pass_info()
    assert info["grad_items"][3] > 0  # the deep gradient pass ran them
    rtol, eps = RTOL[np.dtype(T)], float(np.finfo(T).eps)
    y64 = y.astype(np.float64)
    checked = hand_checked = 0
    po = E.prim_options()
    for t, tree in enumerate(trees):
        lo, hi = flat.const_off[t], flat.const_off[t + 1]
        if hi == lo:
            continue
        xf = srhip.flatten([E.expand(tree, o)], po, dtype=T)
        k, ar, c = xf.tree(0)
        with np.errstate(all="ignore"):
            yh, gc, okt = oracle.eval_grad_consts(k, ar, c.astype(T), X, len(c), dtype=T)
        if not okt:
            continue
        assert ok[t], t
        ref = float(((yh - y) * (yh - y)).astype(np.float64).sum())
        if t >= nhand:
            with np.errstate(all="ignore"):
                spread = loss_spread_flat(xf, X, y, None, T, srhip.L2DistLoss())[0]
            if not 4 * spread <= rtol * abs(ref) + 4 * eps * n:
                continue
        cmap = E.const_map(tree, o)
        assert len(cmap) == len(c) and max(cmap) == hi - lo - 1
        r64 = (yh - y).astype(np.float64)
        seed = 2 * r64
        d = (4 * eps * np.abs(r64)).astype(T).astype(np.float64)
        gc = gc.astype(np.float64)
        G, S, DV = np.zeros(hi - lo), np.zeros(hi - lo), np.zeros(hi - lo)
        for j, i in enumerate(cmap):
            if i < 0:
                continue
            with np.errstate(all="ignore"):
                G[i] += (seed * gc[j]).sum()
                S[i] += np.abs(seed * gc[j]).sum()
                DV[i] += (2 * d * np.abs(gc[j])).sum()
        sel = np.isfinite(S) & (S < 1e20)
        with np.errstate(invalid="ignore"):
            err = np.abs(g[lo:hi] - G)
        bound = rtol * S + DV + 1e-30
        assert np.all(err[sel] <= bound[sel]), (t, srhip.string_tree(tree, o), err[sel].tolist(), bound[sel].tolist())
        assert abs(s[t] - ref) <= rtol * abs(ref) + 4 * eps * n, (t, s[t], ref)
        checked += int(sel.sum())
        hand_checked += int(sel.sum()) if t < nhand else 0
    assert hand_checked == flat.const_off[nhand] == 22  # every constant of the hand-built trees
    assert checked >= 150, checked


@pytest.mark.parametrize("T", DTYPES)
def test_the_other_entries(gpu_ctx, T):
    """Check 4. Per-tree row sets and packed partials with L1 and with an expression loss (E2 of
    tests/expr_loss_cases.py), per-row constant gradients, and new constants followed by an
    evaluation, on the first 60 trees of problem B with narrow features plus the gradient trees."""
    names = E.NONLOSSY + ("dbl", "op2")
    o = E.options(names)
    po = E.prim_options()
    n, bs = 513, 40
    trees = grad_trees(o) + list(srhip.random_population(60, o, 2, T, seed=22, maxsize=15))
    flat = srhip.flatten(trees, o, dtype=T)
    xflat = srhip.flatten([E.expand(t, o) for t in trees], po, dtype=T)
    X = np.random.default_rng(42).standard_normal((2, n)).astype(T)
    y = (np.cos(X[0]) + X[1]).astype(T)
    with np.errstate(all="ignore"):
        yhat, rok = oracle.eval_trees(xflat, X, dtype=T)
    assert rok.sum() >= 50
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = srhip.Program(ctx, flat, T)
    e2 = EL.expr_loss("E2")
    eps = float(np.finfo(T).eps)
    # whole-dataset sums, then the packed partials of the same calls
    from srhip.distributed import pack_partials

    for kind, name in ((L1, None), (e2.kind, "E2")):
        s, ws, ok = prog.eval_loss(ds, kind)
        ok = np.asarray(ok).astype(bool)
        assert ok[rok].all()
        if name is None:
            l = np.abs(yhat - y).astype(np.float64)
            ref, mag = l.sum(axis=1), l.sum(axis=1)
        else:
            ref, mag = EL.reference_sums(name, yhat, y, None, rok, T)
        check_sums(s, ref, mag, float(n), rok & np.isfinite(ref), T, f"{name or 'L1'} {np.dtype(T).name}")
        buf = torch.full((2 * flat.ntrees + 1,), -7.0, dtype=torch.float64, device=f"cuda:{ctx.device}")
        prog.eval_loss_packed(ds, kind, buf.data_ptr())
        ctx.sync()
        np.testing.assert_array_equal(buf.cpu().numpy(), pack_partials(s, ws, ok))
    # per-tree row sets
    rows = np.random.default_rng(43).integers(0, n, (flat.ntrees, bs))
    rows[0, :] = rows[0, 0]
    for kind, name in ((L1, None), (e2.kind, "E2")):
        s, ws, ok = prog.eval_loss_rowsets(ds, kind, rows)
        assert np.allclose(ws, float(bs))
        nchecked = 0
        for t in np.flatnonzero(rok):
            assert ok[t]
            yh, yy = yhat[t][rows[t]], y[rows[t]]
            if name is None:
                lr = np.abs(yh - yy)
            else:
                lr, fin = EL.loss_rows(name, yh, yy, None, T)
                assert fin
            l64 = lr.astype(np.float64)
            assert abs(s[t] - l64.sum()) <= RTOL[np.dtype(T)] * np.abs(l64).sum() + 4 * eps * bs, (name, t)
            nchecked += 1
        assert nchecked >= 50
    # per-row constant gradients: ŷ bit-equal to that of the expansions' gradient program (the same
    # dual-number routines on both sides); ∂ŷ/∂c against the oracle on the expansion (copies summed)
    # within rtol·Σ_copies|∂ŷ/∂c| per row: the bar of the loss sums for the device's own derivative
    # routines, the sum over at most a few copies adding a few ulps
    val, grad, gok = prog.eval_grad_tree_array(ds)
    xval, _, xgok = srhip.Program(ctx, xflat, T).eval_grad_tree_array(ds)
    assert gok[rok].all() and xgok[rok].all()
    rtol = RTOL[np.dtype(T)]
    ngrad = 0
    for t in np.flatnonzero(rok):
        assert np.array_equal(bits(val[t]), bits(xval[t]))
        lo, hi = flat.const_off[t], flat.const_off[t + 1]
        if hi == lo:
            continue
        k, ar, c = xflat.tree(t)
        with np.errstate(all="ignore"):
            _, gc, okt = oracle.eval_grad_consts(k, ar, c.astype(T), X, len(c), dtype=T)
        assert okt
        gc = gc.astype(np.float64)
        G, S = np.zeros((hi - lo, n)), np.zeros((hi - lo, n))
        for j, i in enumerate(E.const_map(trees[t], o)):
            if i >= 0:
                G[i] += gc[j]
                S[i] += np.abs(gc[j])
        fin = np.isfinite(S)
        err = np.abs(grad[lo:hi].astype(np.float64) - G)
        assert np.all(err[fin] <= rtol * S[fin] + 1e-30), (t, srhip.string_tree(trees[t], o))
        ngrad += hi - lo
    assert ngrad >= 100
    # new constants, then an evaluation: the results of a fresh program
    rng = np.random.default_rng(44)
    for it in range(2):
        new = (flat.consts * (1 + 0.3 * rng.standard_normal(len(flat.consts)))).astype(T)
        prog.set_constants(new)
        fresh = srhip.Program(ctx, flat.take(np.arange(flat.ntrees), new), T)
        (va, oka), (vb, okb) = prog.eval_tree_array(ds), fresh.eval_tree_array(ds)
        assert np.array_equal(oka, okb) and oka.sum() >= 40 and np.array_equal(bits(va[oka]), bits(vb[oka]))
        sa, ga, _, oka = prog.eval_loss_grad(ds, L2)
        sb, gb, _, okb = fresh.eval_loss_grad(ds, L2)
        assert np.array_equal(oka, okb) and np.array_equal(sa, sb, equal_nan=True) and np.array_equal(ga, gb, equal_nan=True)
    st = prog.update_stats()
    assert st["inplace"] >= 1, st


def test_constant_optimisation_lowers_the_loss(gpu_ctx):
    """Check 4, srhip_optimize_constants_batch: on y = 2·custom_cos(x1 + 0.5), starts
    c1·custom_cos(x1 + c2) away from the solution; no returned loss exceeds its start and the
    best one falls by more than half."""
    T, n = np.float32, 513
    o = E.options(("custom_cos",))
    cc = E.expr_op("custom_cos")
    X = np.random.default_rng(51).standard_normal((1, n)).astype(T)
    y = np.array([2 * op_eval(T, cc, T(v) + T(0.5)) for v in X[0]], dtype=T)
    starts = [(1.0, 0.2), (1.5, 0.9), (2.5, 0.4), (0.5, 0.5)]
    trees = [o.make_binary("*", Node(val=a), o.make_unary("custom_cos", o.make_binary("+", Node("x1"), Node(val=b))))
             for a, b in starts]
    opts = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", cc])  # as o
    ds = srhip.Dataset(X, y)
    start, ok = srhip.eval_loss_batch_ok(trees, ds, opts)
    assert ok.all() and (start > 1e-3).all()
    res = srhip.optimize_constants_batch(ds, trees, opts, rng=np.random.default_rng(52))
    got = np.asarray(res.losses).astype(T)
    assert np.all(got <= start), (got, start)
    assert got.min() < 0.5 * start.min() or got.min() < 1e-6, (got, start)
    after, ok = srhip.eval_loss_batch_ok(trees, ds, opts)  # the trees were updated in place
    assert ok.all() and np.all(after <= start)


def test_placement(gpu_ctx):
    """Check 5. Shallow operator trees all go to the deep list. In a default-jit program of 300
    primitive trees plus operator trees the primitive ones keep their tree code, and their results
    are bit-equal to those of the program without the operator trees."""
    T, n = np.float32, 513
    o = E.options(E.NONLOSSY)
    U, B = o.make_unary, o.make_binary
    small = [U("custom_cos", Node("x1")), B("my_func_a", Node("x1"), Node("x2")), B("my_func_c", Node("x1"), Node(val=2.0)),
             U("op3", B("+", Node("x1"), Node("x2")))]
    ctx = gpu_ctx
    prog = srhip.Program(ctx, srhip.flatten(small, o, dtype=T), T)
    info = prog.pass_info()
    assert (info["shallow"], info["deep"]) == (0, len(small)), info
    po = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    prims = list(srhip.random_population(300, po, 2, T, seed=61, maxsize=15))  # op indices are o's too
    X = np.random.default_rng(62).standard_normal((2, n)).astype(T)
    y = (np.cos(X[0]) + X[1]).astype(T)
    ds = srhip.DeviceDataset(ctx, X, y)
    base = srhip.Program(ctx, srhip.flatten(prims, o, dtype=T), T)
    mixed = srhip.Program(ctx, srhip.flatten(prims + small, o, dtype=T), T)
    bi, mi = base.pass_info(), mixed.pass_info()
    assert bi["tree_code"] >= 256 and mi["tree_code"] == bi["tree_code"], (bi, mi)
    assert mi["deep"] == bi["deep"] + len(small) and mi["shallow"] == bi["shallow"]
    sb, _, okb = base.eval_loss(ds, L2)
    assert ctx.last_tree_code() == bi["tree_code"]
    sm, _, okm = mixed.eval_loss(ds, L2)
    assert ctx.last_tree_code() == bi["tree_code"]
    assert np.array_equal(okb, okm[:300]) and np.array_equal(sb, sm[:300], equal_nan=True)
    assert np.asarray(okm[300:]).all() and np.isfinite(sm[300:]).all()
    # gradients: the operator trees stay out of the gradient tree code
    gb = base.eval_loss_grad(ds, L2)
    njit = ctx.last_tree_code()
    gm = mixed.eval_loss_grad(ds, L2)
    assert ctx.last_tree_code() == njit
    nc = len(gb[1])
    assert np.array_equal(gb[0], gm[0][:300], equal_nan=True) and np.array_equal(gb[1], gm[1][:nc], equal_nan=True)


def test_handle_lifetime(gpu_ctx):
    """Check 6. A program holds its definitions: after the handle is destroyed it still evaluates
    (also after new constants, which compile trees again), and creating a new program is an
    invalid argument."""
    T, n = np.float32, 256
    po = E.prim_options()
    op = srhip.ExprOp("tmp_dbl", E.dbl(po), po, 1)
    o = srhip.Options(binary_operators=["+", "*"], unary_operators=["cos", op])
    trees = [o.make_unary("tmp_dbl", o.make_binary("*", Node(val=0.7), Node("x1"))),
             o.make_binary("+", Node("x1"), o.make_unary("tmp_dbl", Node(val=1.5)))]
    flat = srhip.flatten(trees, o, dtype=T)
    X = np.random.default_rng(71).standard_normal((1, n)).astype(T)
    ctx = gpu_ctx
    ds = srhip.DeviceDataset(ctx, X, np.zeros(n, dtype=T))
    prog = srhip.Program(ctx, flat, T)
    before, ok = prog.eval_tree_array(ds)
    assert ok.all()
    u = (T(0.7) * X[0]).astype(T)
    assert np.array_equal(bits(before[0]), bits((u * u + u).astype(T)))
    assert np.array_equal(bits(before[1]), bits((X[0] + T(3.75)).astype(T)))
    op.destroy()
    after, ok = prog.eval_tree_array(ds)
    assert ok.all() and np.array_equal(bits(after), bits(before))
    prog.set_constants(np.array([0.5, np.inf], dtype=T))  # tree 1's fold is now non-finite: compiled again
    out, ok = prog.eval_tree_array(ds)
    assert ok.tolist() == [True, False]
    u = (T(0.5) * X[0]).astype(T)
    assert np.array_equal(bits(out[0]), bits((u * u + u).astype(T)))
    s, g, _, gok = prog.eval_loss_grad(ds, L2)
    assert gok.tolist() == [True, False] and np.isfinite(g[0])
    with pytest.raises(srhip.SrhipError) as err:
        srhip.Program(ctx, flat, T)
    assert err.value.code == _lib.ERR_INVALID and not isinstance(err.value, srhip.Unsupported)
