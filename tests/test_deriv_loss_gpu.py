"""Derivative objectives on the engine (srhip_eval_loss_deriv): one
table loss reduced on ŷ and on ∂ŷ/∂x_d per direction, for a whole batch in one pass
of the forward-mode interpreter with tangents seeded at feature leaves.

Reference: per-row ŷ and ∂ŷ/∂x from the Float64 oracle's forward mode on the
`x + (-0.0)`-seeded tree, as test_engine_feature_gradients_vs_oracle_random builds
it. Bounds of a derivative channel's sum (tests 2, 3, 5, 6, 9), with r_i the
reference residual and δ_i the per-row bound on the derivative's error:
  L2:          |sum − ref| ≤ Σ_i w_i (2|r_i| δ_i + δ_i²) + bar · Σ_i w_i r_i²
  L1, Huber(1) |sum − ref| ≤ Σ_i w_i δ_i + bar · ref        (|dℓ/dr| ≤ 1)
δ_i = rtol·|d_i| + atol + 4·spread_i with the rtol / atol of the existing
feature-gradient tests (Float64 1e-11 / 1e-11, test_engine_feature_gradients_vs_oracle_random;
Float32 2e-4 / 2e-4, test_engine_feature_derivatives_kat) and grad_spread's per-row
spread (a row whose loss overflows T, computed in T as the reference computes it, must
give a non-finite sum instead); bar is the sum bar of channel 0 (Float32 1e-5, the project's bar; Float64
1e-10, test_gpu_parity.py test_float64_parity's losses).

Row counts: 300 (a partial last tile at every R) and 1025, the smallest count at
which every variant's plan has more than one row group (the largest workgroup
covers 1024 rows; checked through srhip_last_loss_launch)."""
import ctypes as C
import functools

import numpy as np
import pytest

import expr_loss_cases as EL
import expr_op_cases as EO
import oracle
import srhip
from numerics import assert_close_conditioned, loss_spread
from srhip import Node, _lib
from srhip import constants as K
from srhip.engine import MultiDeviceDataset, Program
from srhip.interface import _seed_features
from test_gradients import grad_spread

pytestmark = pytest.mark.gpu

RTOL = {np.float64: 1e-11, np.float32: 2e-4}  # per-row derivative bounds of the feature-gradient tests
KAT = {np.float64: 1e-9, np.float32: 2e-4}  # test_engine_feature_derivatives_kat's rtol = atol
BAR = {np.float64: 1e-10, np.float32: 1e-5}  # sum bars of the loss parity tests
L2, L1, HUBER = K.LOSS["L2"], K.LOSS["L1"], K.LOSS["HUBER"]


# ---- shared references --------------------------------------------------------------
def _pop_options():
    return srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])


@functools.lru_cache(maxsize=None)
def population(T):
    """Test 3's population with its per-row reference, computed once per dtype:
    (options, trees, X in T, per tree (ŷ, ∂ŷ/∂x [4, n], ok, spread [4, n]))."""
    o = _pop_options()
    trees = srhip.random_population(200, o, 4, T, seed=91)
    X = np.random.default_rng(92).standard_normal((4, 300)).astype(T)
    return o, trees, X, [row_reference(t, o, X, T) for t in trees]


def row_reference(tree, o, X, T):
    """(ŷ [n], ∂ŷ/∂x [nfeat, n], ok, spread of ∂ŷ/∂x [nfeat, n]) from the Float64 oracle on
    the seeded tree (constants rounded to T)."""
    binops = tuple(o.binary_operators)
    if "+" in binops:
        oo, plus = o, binops.index("+") + 1
    else:
        oo, plus = srhip.Options(binary_operators=binops + ("+",), unary_operators=o.unary_operators), len(binops) + 1
    aug, seeds = _seed_features(tree, plus, None)
    v, g, ok, _, sg = grad_spread(aug, oo, X, T)
    seeds = np.asarray(seeds)
    nfeat, n = X.shape
    D, S = np.zeros((nfeat, n)), np.zeros((nfeat, n))
    for f in range(1, nfeat + 1):
        m = seeds == f
        if m.any():
            D[f - 1] = g[m].sum(axis=0)
            S[f - 1] = sg[m].sum(axis=0)
    return v, D, bool(ok), S


def channel_bound(kind, param, d, tgt, w, delta, bar):
    """(reference Σ w·ℓ(d, tgt), the bound on the engine's sum) of one derivative channel."""
    w = np.ones_like(d) if w is None else np.asarray(w, dtype=np.float64)
    r = d - np.asarray(tgt, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == L2:
            ref = np.sum(w * r * r)
            return ref, np.sum(w * (2 * np.abs(r) * delta + delta * delta)) + bar * ref
        rows = np.asarray([oracle.elem_loss(kind, [param], float(a), float(b), dtype=np.float64)
                           for a, b in zip(d, np.asarray(tgt, dtype=np.float64))])
        ref = np.sum(w * rows)
        return ref, np.sum(w * delta) + bar * ref


def check_channels(sums, ok, refs, dirs, Y, W, T, kind=L2, param=0.0, rtol=None, use_spread=True, msg=""):
    """Every derivative channel of every succeeding tree within its bound; returns the count."""
    rtol = RTOL[T] if rtol is None else rtol
    n = 0
    for t, (v, D, rok, S) in enumerate(refs):
        if not ok[t]:
            continue
        for j, d in enumerate(dirs):
            dd = D[d - 1]
            delta = rtol * np.abs(dd) + rtol + (4 * S[d - 1] if use_spread else 0.0)
            ref, tol = channel_bound(kind, param, dd, Y[1 + j], None if W is None else W[1 + j], delta, BAR[T])
            got = sums[t, 1 + j]
            print(f"{msg} tree {t} dir {d}: sum {got!r} ref {ref!r} err {abs(got - ref):.3e} tol {tol:.3e}")
            n += 1
            # the loss is computed in T (the reference's rule): a finite derivative whose row loss
            # overflows T gives a non-finite sum there, and must give one here
            with np.errstate(all="ignore"):
                rT = dd.astype(T) - Y[1 + j]
                lT = rT * rT if kind == L2 else np.abs(rT)
            if not np.isfinite(lT).all():
                assert not np.isfinite(got), (msg, t, d, got, ref)
                continue
            if ref > np.finfo(T).max and not np.isfinite(got):
                continue  # the sum itself is beyond T: a partial sum in T may overflow
            assert abs(got - ref) <= tol or not np.isfinite(tol), (msg, t, d, got, ref, tol)
    return n


def make_targets(X, dirs, T, seed):
    """y and one derivative target per direction, and per-channel weights."""
    rng = np.random.default_rng(seed)
    n = X.shape[1]
    Y = rng.standard_normal((1 + len(dirs), n)).astype(T)
    W = rng.uniform(0.5, 1.5, (1 + len(dirs), n)).astype(T)
    return Y, W


def run_deriv(ctx, trees, o, X, Y, W, dirs, T, kind=L2, params=None):
    """Program.eval_loss_deriv on a MultiDeviceDataset: (sums, wsum, ok)."""
    ds = MultiDeviceDataset(ctx, X, Y, W)
    prog = Program(ctx, srhip.flatten(trees, o, dtype=T), T, interpreted=True)
    return prog.eval_loss_deriv(ds, kind, [d - 1 for d in dirs], params)


# ---- 1. exact cases --------------------------------------------------------------------
def exact_trees(o):
    B = o.make_binary
    x1, x2 = (lambda: Node("x1")), (lambda: Node("x2"))
    return [B("+", B("*", x1(), x1()), B("*", Node(val=3.0), x2())),  # x1*x1 + 3*x2
            B("-", B("*", x1(), x2()), B("*", x2(), x2())),  # x1*x2 - x2*x2
            B("*", Node(val=2.0), x1()),  # 2*x1
            Node(val=2.0)]


def exact_rows(X):
    """Per tree (ŷ, ∂ŷ/∂x [3, n]) in exact integer arithmetic."""
    x1, x2 = X[0], X[1]
    z, one = np.zeros_like(x1), np.ones_like(x1)
    return [(x1 * x1 + 3 * x2, [2 * x1, 3 * one, z]),
            (x1 * x2 - x2 * x2, [x2, x1 - 2 * x2, z]),
            (2 * x1, [2 * one, z, z]),
            (2 * one, [z, z, z])]


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("n", [300, 1025])
@pytest.mark.parametrize("weighted", [False, True])
def test_exact_integer_cases(gpu_ctx, T, n, weighted):
    """Small-integer X, targets and weights, L2: every channel sum is an integer below
    2^24 and must equal numpy's bit for bit. Pins the V_XX double seed, the left and
    right operand seeds, unused slots (direction 3 is in no tree: Σ w·ℓ(0, g)), constants
    that seed nothing (2*x1) and the column order."""
    o = srhip.Options(binary_operators=["+", "-", "*"], unary_operators=[])
    rng = np.random.default_rng(5)
    X = rng.integers(1, 5, (4, n)).astype(np.float64)
    rows = exact_rows(X)
    for dirs in ([1], [2, 1], [1, 2, 3]):
        Y = rng.integers(-3, 4, (1 + len(dirs), n)).astype(np.float64)
        W = rng.integers(1, 4, (1 + len(dirs), n)).astype(np.float64) if weighted else None
        sums, wsum, ok = run_deriv(gpu_ctx, exact_trees(o), o, X.astype(T), Y.astype(T), None if W is None else W.astype(T),
                                   dirs, T)
        assert gpu_ctx.last_kernel_name() == ("grad_kernel_deriv<float>" if T == np.float32 else "grad_kernel_deriv<double>")
        assert gpu_ctx.last_tree_code() == 0
        if n == 1025:
            assert gpu_ctx.last_loss_launch()["nrg"] > 1
        assert ok.all()
        Wn = np.ones_like(Y) if W is None else W
        assert np.array_equal(wsum, Wn.sum(axis=1))
        for t, (v, D) in enumerate(rows):
            want = [np.sum(Wn[0] * (v - Y[0]) ** 2)] + [np.sum(Wn[1 + j] * (D[d - 1] - Y[1 + j]) ** 2)
                                                          for j, d in enumerate(dirs)]
            assert max(want) < 2 ** 24
            assert np.array_equal(sums[t], np.asarray(want)), (dirs, t, sums[t], want)


# ---- 2. an operator set without "+" ---------------------------------------------------
@pytest.mark.parametrize("T", [np.float64, np.float32])
def test_operator_set_without_plus(gpu_ctx, T):
    """cos(x1*x2)/x1 under ["*", "/"], ["cos"] against the analytic derivative, within
    test_engine_feature_derivatives_kat's per-row bounds carried into the sum."""
    o = srhip.Options(binary_operators=["*", "/"], unary_operators=["cos"])
    tree = o.make_binary("/", o.make_unary("cos", o.make_binary("*", Node("x1"), Node("x2"))), Node("x1"))
    X = (np.random.default_rng(0).random((4, 300)) * 5 + 0.1).astype(T)
    x1, x2 = X[0].astype(np.float64), X[1].astype(np.float64)
    D = np.zeros((4, 300))
    D[0] = -np.sin(x1 * x2) * x2 / x1 - np.cos(x1 * x2) / x1 ** 2
    D[1] = -np.sin(x1 * x2)
    dirs = [1, 2, 3]
    Y, W = make_targets(X, dirs, T, 1)
    sums, wsum, ok = run_deriv(gpu_ctx, [tree], o, X, Y, W, dirs, T)
    assert ok.all() and np.isfinite(sums).all()
    refs = [(np.cos(x1 * x2) / x1, D, True, np.zeros((4, 300)))]
    assert check_channels(sums, ok, refs, dirs, Y, W, T, rtol=KAT[T], use_spread=False, msg="no-plus") == 3
    v = refs[0][0]  # the value channel, by the same rule
    ref0, tol0 = channel_bound(L2, 0.0, v, Y[0], W[0], KAT[T] * np.abs(v) + KAT[T], BAR[T])
    assert abs(sums[0, 0] - ref0) <= tol0


# ---- 3. random population against the Float64 oracle ------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("dirs", [[1, 2, 3, 4], [2]])
@pytest.mark.parametrize("weighted", [False, True])
def test_random_population_vs_oracle(gpu_ctx, T, dirs, weighted):
    o, trees, X, refs = population(T)
    Y, W = make_targets(X, dirs, T, 93)
    W = W if weighted else None
    dds = srhip.DerivativeDataset(X, Y[0], Y[1:], dirs, W)
    means, ok = srhip.eval_deriv_loss_batch(trees, dds, o)
    wsum = np.full(1 + len(dirs), 300.0) if W is None else W.astype(np.float64).sum(axis=1)
    sums = means * wsum
    # the flags are those of the value evaluation
    _, ok0 = srhip.eval_loss_batch_ok(trees, dds.target(0), o)
    assert np.array_equal(ok, ok0)
    assert np.isnan(means[~ok]).all()
    # conditions on the population, not measurements
    nok = int(ok.sum())
    assert nok >= 150 and 200 - nok >= 5
    for t in np.flatnonzero(ok):
        assert refs[t][2] and np.isfinite(refs[t][1]).all(), t
    uses = np.zeros(4, dtype=int)
    for tr in trees:
        uses += np.asarray([f"x{f}" in srhip.string_tree(tr, o) for f in range(1, 5)])
    assert uses.min() >= 93, uses
    # channel 0: the loss parity tests' bar (relative, plus the oracle's own spread)
    flat = srhip.flatten(trees, o, dtype=T)
    w0 = None if W is None else W[0]
    ref0, _, rok = oracle.eval_loss_batch(flat, X, Y[0], w0, dtype=T)
    sp = loss_spread(trees, o, X, Y[0], w0, T)
    m = ok & rok & np.isfinite(ref0)
    assert m.sum() >= 150
    assert_close_conditioned(sums[m, 0], ref0[m], sp[m], rtol=BAR[T], msg="channel 0")
    # derivative channels: no tree left out
    assert check_channels(sums, ok, refs, dirs, Y, W, T, msg=f"random {T.__name__}") == nok * len(dirs)


# ---- 4. tangent groups ------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_tangent_groups_permutation(gpu_ctx, T):
    """ndir = 5 on 6 features runs two tangent groups. The ndir = 1 launch carries one
    tangent with another R (Float32: 4 rows per lane against 2), so the second of the
    issue's two forms holds: directions [d5, d1, d2, d3, d4] equal [d1..d5] permuted,
    channel by channel and bit for bit (a channel's arithmetic does not depend on its slot
    or group)."""
    o = _pop_options()
    trees = srhip.random_population(40, o, 6, T, seed=94)
    X = np.random.default_rng(95).standard_normal((6, 300)).astype(T)
    d = [2, 5, 1, 6, 3]
    Y, W = make_targets(X, d, T, 96)
    a, wa, oka = run_deriv(gpu_ctx, trees, o, X, Y, W, d, T)
    perm = [4, 0, 1, 2, 3]
    cols = [0] + [1 + k for k in perm]
    b, wb, okb = run_deriv(gpu_ctx, trees, o, X, Y[cols], W[cols], [d[k] for k in perm], T)
    assert np.array_equal(oka, okb) and oka.sum() >= 20
    assert np.array_equal(wa[cols], wb)
    assert np.array_equal(a[:, cols], b, equal_nan=True)
    # and the groups hold what a 4-direction call holds, within the bounds of test 3
    refs = [row_reference(t, o, X, T) for t in trees[:10]]
    assert check_channels(a[:10], oka[:10], refs, d, Y, W, T, msg="groups") == int(oka[:10].sum()) * 5


# ---- 5. deep and wide ---------------------------------------------------------------------
def deep_tree(o, depth=6):
    """A full binary tree: more live values than the shallow variant has slots."""
    leaves = iter(range(10 ** 6))

    def rec(d):
        if d == 0:
            k = next(leaves)
            return Node(f"x{1 + k % 4}") if k % 5 else Node(val=0.5 + 0.25 * (k % 3))
        return o.make_binary("*" if d % 2 else "+", rec(d - 1), rec(d - 1))

    return o.make_unary("cos", rec(depth))


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_deep_variant(gpu_ctx, T):
    o = _pop_options()
    trees = [deep_tree(o), o.make_binary("*", Node("x1"), Node("x2"))]
    X = (np.random.default_rng(97).random((4, 300)) + 0.5).astype(T)
    dirs = [3, 1]
    Y, W = make_targets(X, dirs, T, 98)
    ds = MultiDeviceDataset(gpu_ctx, X, Y, W)
    prog = Program(gpu_ctx, srhip.flatten(trees, o, dtype=T), T, interpreted=True)
    sums, wsum, ok = prog.eval_loss_deriv(ds, L2, [d - 1 for d in dirs])
    assert prog.pass_info()["grad_items"][3] >= 1  # the first tree is a deep program
    assert gpu_ctx.last_kernel_name() == ("grad_kernel_deriv<float>" if T == np.float32 else "grad_kernel_deriv<double>")
    assert ok.all()
    refs = [row_reference(t, o, X, T) for t in trees]
    assert check_channels(sums, ok, refs, dirs, Y, W, T, msg="deep") == 4


@pytest.mark.parametrize("nfeat,force", [(90, True), (330, False)], ids=["90-SRHIP_WIDE=1", "330"])
def test_wide_variant(gpu_ctx, monkeypatch, nfeat, force):
    """The variant that reads its features from global memory. The gradient kernels' row
    tile is 128 or 256 Float32 rows, so 90 features still fit in LDS there (the loss
    kernels' 512-row tile does not): that dataset runs wide under SRHIP_WIDE=1 (read per
    call), as the other wide gradient tests force it, and 330 features x 8 columns run
    wide on their own (no tile of 128 rows fits 160 KiB)."""
    T = np.float32
    o = _pop_options()
    trees = srhip.random_population(24, o, nfeat, T, seed=99)
    B = o.make_binary
    last, mid = f"x{nfeat}", f"x{nfeat // 2}"
    trees += [B("*", Node(last), B("+", Node(mid), Node(last))), o.make_unary("cos", B("*", Node("x1"), Node(last)))]
    X = np.random.default_rng(100).standard_normal((nfeat, 300)).astype(T)
    dirs = [nfeat, nfeat // 2, 1]
    Y, W = make_targets(X, dirs, T, 101)
    if force:
        sums0, _, ok0 = run_deriv(gpu_ctx, trees, o, X, Y, W, dirs, T)
        assert gpu_ctx.last_kernel_name() == "grad_kernel_deriv<float>"
        monkeypatch.setenv("SRHIP_WIDE", "1")
    sums, wsum, ok = run_deriv(gpu_ctx, trees, o, X, Y, W, dirs, T)
    assert gpu_ctx.last_kernel_name() == "grad_kernel_wide_deriv<float>"
    assert gpu_ctx.last_tree_code() == 0
    assert ok.sum() >= 12 and ok[-2:].all()
    if force:
        assert np.array_equal(ok, ok0)
    refs = [row_reference(t, o, X, T) for t in trees]
    assert check_channels(sums, ok, refs, dirs, Y, W, T, msg="wide") == int(ok.sum()) * 3


# ---- 6. other table losses -------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("loss", [(L1, 0.0), (HUBER, 1.0)])
def test_l1_and_huber_channel(gpu_ctx, T, loss):
    o, trees, X, refs = population(T)
    kind, param = loss
    dirs = [2]
    Y, W = make_targets(X, dirs, T, 102)
    sums, wsum, ok = run_deriv(gpu_ctx, trees, o, X, Y, W, dirs, T, kind, [param])
    assert ok.sum() >= 150
    assert check_channels(sums, ok, refs, dirs, Y, W, T, kind, param, msg=f"loss {kind}") == int(ok.sum())


# ---- 7. non-finite derivative ---------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_non_finite_derivative_keeps_ok(gpu_ctx, T):
    """safe_sqrt(x1) at x1 = 0: the value is finite, the derivative is not. The engine's
    rule: ok = 1, channel 0 finite, channel 1 non-finite; the objective is +Inf."""
    o = srhip.Options(binary_operators=["+", "*"], unary_operators=["safe_sqrt"])
    tree = o.make_unary("safe_sqrt", Node("x1"))
    X = np.zeros((2, 300), dtype=T)
    X[0, 1:] = np.linspace(0.5, 2.0, 299)
    dds = srhip.DerivativeDataset(X, np.ones(300, dtype=T), np.ones((1, 300), dtype=T), [1])
    means, ok = srhip.eval_deriv_loss_batch([tree], dds, o)
    assert ok[0] and np.isfinite(means[0, 0]) and not np.isfinite(means[0, 1])
    oo = srhip.Options(binary_operators=["+", "*"], unary_operators=["safe_sqrt"],
                       loss_function=srhip.DerivativeObjective([1.0, 1.0]))
    losses, lok = srhip.eval_loss_batch_ok([tree], dds, oo)
    assert losses[0] == np.inf and not lok[0]


# ---- 8. ABI errors -----------------------------------------------------------------------
def test_abi_errors_before_any_launch():
    """Each refusal of srhip.h's table returns its code, leaves the outputs untouched and
    launches nothing (a context of its own, whose launch count stays 0)."""
    T = np.float32
    ctx = srhip.Context(0)
    ds = prog = xprog = None
    try:
        o = _pop_options()
        X = np.random.default_rng(1).standard_normal((4, 64)).astype(T)
        Y = np.zeros((3, 64), dtype=T)
        ds = MultiDeviceDataset(ctx, X, Y)
        prog = Program(ctx, srhip.flatten([o.make_binary("*", Node("x1"), Node("x2"))], o, dtype=T), T, interpreted=True)
        xo = EO.options(("dbl",))
        xprog = Program(ctx, srhip.flatten([xo.make_unary("dbl", Node("x1"))], xo, dtype=T), T, interpreted=True)
        L = _lib.lib()
        huber = np.asarray([1.0])

        def call(p, kind, dirs, ndir=None, dataset=ds, null_dir=False, params=huber):
            d = np.asarray(dirs, dtype=np.int32)
            sums = np.full(8, -7.0)
            wsum = np.full(8, -7.0)
            ok = np.full(4, 9, dtype=np.uint8)
            rc = L.srhip_eval_loss_deriv(dataset.handle, p.handle, kind, params.ctypes.data,
                                         None if null_dir else d.ctypes.data, len(d) if ndir is None else ndir,
                                         sums.ctypes.data, wsum.ctypes.data, ok.ctypes.data)
            assert (sums == -7.0).all() and (wsum == -7.0).all() and (ok == 9).all()
            return rc

        INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
        assert call(prog, L2, [0, 1], null_dir=True) == INV
        assert call(prog, L2, [], ndir=0) == INV
        assert call(prog, L2, list(range(16)), ndir=16) == INV
        assert call(prog, L2, [0]) == INV  # 3 columns, 1 direction
        assert call(prog, L2, [0, 1, 2]) == INV
        assert call(prog, L2, [0, 4]) == INV
        assert call(prog, L2, [-1, 0]) == INV
        assert call(prog, L2, [1, 1]) == INV
        assert call(prog, K.MARGIN_LOSS_BEGIN, [0, 1]) == INV
        assert call(prog, K.LOSS["DWDMARGIN"], [0, 1]) == INV
        assert call(prog, EL.expr_loss("SQ").kind, [0, 1]) == UNS
        assert call(xprog, L2, [0, 1]) == UNS
        assert ctx.last_kernel_time()[1] == 0
        # and the accepted call launches
        sums, wsum, ok = prog.eval_loss_deriv(ds, L2, [0, 1])
        assert ctx.last_kernel_time()[1] >= 1 and ok.all()
    finally:
        for obj in (prog, xprog, ds):  # destroyed now, before their context is closed
            if obj is not None:
                obj.__del__()
        ctx.close()


# ---- 9. the objective end to end ---------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_objective_end_to_end(gpu_ctx, T):
    o, trees, X, refs = population(T)
    dirs = [1, 3]
    Y, W = make_targets(X, dirs, T, 103)
    dds = srhip.DerivativeDataset(X, Y[0], Y[1:], dirs, W)
    coef = [1.0, 0.5, 0.25]
    obj = srhip.DerivativeObjective(coef)
    oo = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"], loss_function=obj)
    losses, ok = srhip.eval_loss_batch_ok(trees, dds, oo)
    means, mok = srhip.eval_deriv_loss_batch(trees, dds, oo)
    with np.errstate(all="ignore"):
        comb = means @ np.asarray(coef)
    fin = mok & np.isfinite(comb)
    assert np.array_equal(ok, fin) and losses.dtype == T
    assert np.array_equal(losses[fin], comb[fin].astype(T)) and (losses[~fin] == np.inf).all()
    assert np.array_equal(srhip.eval_loss_batch(trees, dds, oo), losses)
    # the objective's own per-tree call (eval_tree_array + eval_diff_tree_array) agrees within the channel
    # bounds: each mean within its bound / Σw of the reference, twice (both sides carry the error)
    wsum = W.astype(np.float64).sum(axis=1)
    picked = [t for t in range(len(trees)) if fin[t]][:12]
    for t in picked:
        single = obj(trees[t], dds, oo)
        tol = 0.0
        v, D, _, S = refs[t]
        r0 = np.sum(W[0].astype(np.float64) * (v - Y[0]) ** 2)
        tol += coef[0] * 2 * (BAR[T] * r0 + 4 * loss_spread([trees[t]], o, X, Y[0], W[0], T)[0]) / wsum[0]
        for j, d in enumerate(dirs):
            delta = RTOL[T] * np.abs(D[d - 1]) + RTOL[T] + 4 * S[d - 1]
            _, b = channel_bound(L2, 0.0, D[d - 1], Y[1 + j], W[1 + j], delta, BAR[T])
            tol += coef[1 + j] * 2 * b / wsum[1 + j]
        tol += 4 * np.finfo(T).eps * abs(comb[t])  # the two casts to T
        print(f"objective tree {t}: batch {losses[t]!r} single {single!r} tol {tol:.3e}")
        assert abs(float(single) - float(losses[t])) <= tol or not np.isfinite(tol), (t, single, losses[t], tol)
    with pytest.raises(ValueError, match="not supported"):
        srhip.optimize_constants_batch(dds, trees[:2], oo)
