"""Constant gradients and optimisation under a derivative objective:
srhip_eval_loss_grad_deriv, srhip_eval_mixed_tree_array's sums' side, and
srhip_optimize_constants_deriv.

Bounds of the fixture test (nothing fitted to the engine's results). Per row, the bound on a
derivative d and on a mixed partial m is the one test_deriv_loss_gpu.py uses for d:
  δ(v) = RTOL[T]·|v| + RTOL[T] + 4·spread(v)
with the spread stored in tests/golden/deriv_grad_cases.npz (the movement of the mpmath value
under a 4-ulp-of-T move of the operands, kept as the next power of two). A channel's gradient sum is Σ_i w_i ℓ'(d_i − g_i)·m_i
with ℓ' = 2r for L2, so with r the reference residual
  |sum − ref| ≤ Σ_i w_i (2 δ(d)_i (|m_i| + δ(m)_i) + 2 |r_i| δ(m)_i) + BAR[T]·Σ_i w_i |2 r_i m_i|
(channel 0 likewise with ŷ and ∂ŷ/∂c, whose per-row bounds are the same form). BAR is
test_deriv_loss_gpu.BAR, the sum bar, on Σ|terms|.

Row counts: 300 (a partial last tile at every R) and 1025, the smallest count at which every
variant's plan has more than one row group: the row tile is the one srhip_eval_loss_deriv's
variant of the same call has (R = 4, 2 or 1 rows per lane; kernels.hip plan_geometry doubles the
tiles of a workgroup while they stay within 8192 rows, 16 tiles and 40 KiB), so the largest
workgroup still covers 1024 rows; checked through srhip_last_loss_launch."""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest

import expr_loss_cases as EL
import expr_op_cases as EO
import srhip
from srhip import Node, _lib
from srhip import constants as K
from srhip.engine import MultiDeviceDataset, Program
from test_deriv_loss_gpu import BAR, RTOL, deep_tree, make_targets

pytestmark = pytest.mark.gpu

L2, L1, HUBER = K.LOSS["L2"], K.LOSS["L1"], K.LOSS["HUBER"]
GOLDEN = Path(__file__).resolve().parent / "golden"
TIDS = dict(ids=lambda T: np.dtype(T).name)


def kname(T):
    return "grad_kernel_deriv2<float>" if T == np.float32 else "grad_kernel_deriv2<double>"


def run_grad(ctx, trees, o, X, Y, W, dirs, T, kind=L2, params=None):
    """(Program.eval_loss_grad_deriv, Program.eval_loss_deriv) on one MultiDeviceDataset."""
    ds = MultiDeviceDataset(ctx, X, Y, W)
    prog = Program(ctx, srhip.flatten(trees, o, dtype=T), T, interpreted=True)
    d0 = [d - 1 for d in dirs]
    plain = prog.eval_loss_deriv(ds, kind, d0, params)
    got = prog.eval_loss_grad_deriv(ds, kind, d0, params)
    return got, plain


# ---- 1. exact cases ----------------------------------------------------------------------
C1, C2 = 2.0, 3.0


def exact_trees(o):
    B = o.make_binary
    x1, x2 = (lambda: Node("x1")), (lambda: Node("x2"))
    return [B("+", B("*", B("*", Node(val=C1), x1()), x1()), B("*", B("*", Node(val=C2), x1()), x2())),
            B("-", B("*", Node(val=C1), x1()), B("*", B("*", Node(val=C2), x2()), x2())),
            B("*", Node(val=C1), x1()),
            Node(val=C1)]


def exact_rows(X):
    """Per tree (ŷ, ∂ŷ/∂c [nc], ∂ŷ/∂x [3], ∂²ŷ/∂x∂c [3][nc]) in exact integer arithmetic."""
    x1, x2 = X[0], X[1]
    z, one = np.zeros_like(x1), np.ones_like(x1)
    return [(C1 * x1 * x1 + C2 * x1 * x2, [x1 * x1, x1 * x2], [2 * C1 * x1 + C2 * x2, C2 * x1, z],
             [[2 * x1, x2], [z, x1], [z, z]]),
            (C1 * x1 - C2 * x2 * x2, [x1, -x2 * x2], [C1 * one, -2 * C2 * x2, z], [[one, z], [z, -2 * x2], [z, z]]),
            (C1 * x1, [x1], [C1 * one, z, z], [[one], [z], [z]]),
            (C1 * one, [one], [z, z, z], [[z], [z], [z]])]


@pytest.mark.parametrize("T", [np.float32, np.float64], **TIDS)
@pytest.mark.parametrize("n", [300, 1025])
@pytest.mark.parametrize("weighted", [False, True])
def test_exact_integer_cases(gpu_ctx, T, n, weighted):
    """Small-integer X, targets, weights and constants, L2: every loss sum and gradient sum is an
    integer below 2^24 and must equal numpy's bit for bit. Pins the seeds of both kinds at every
    operand position these trees have, the channel-0 sums riding on the first direction's
    items, a constant-only tree, and the output layout."""
    o = srhip.Options(binary_operators=["+", "-", "*"], unary_operators=[])
    rng = np.random.default_rng(5)
    X = rng.integers(1, 4, (4, n)).astype(np.float64)
    rows = exact_rows(X)
    for dirs in ([1], [2, 1], [1, 2, 3]):
        Y = rng.integers(-3, 4, (1 + len(dirs), n)).astype(np.float64)
        Y[0] += 20  # keeps channel 0's residuals small
        W = rng.integers(1, 3, (1 + len(dirs), n)).astype(np.float64) if weighted else None
        (sums, grads, wsum, ok), (psums, pwsum, pok) = run_grad(
            gpu_ctx, exact_trees(o), o, X.astype(T), Y.astype(T), None if W is None else W.astype(T), dirs, T)
        assert gpu_ctx.last_kernel_name() == kname(T)
        assert gpu_ctx.last_tree_code() == 0
        if n == 1025:
            assert gpu_ctx.last_loss_launch()["nrg"] > 1
        assert ok.all() and pok.all()
        Wn = np.ones_like(Y) if W is None else W
        assert np.array_equal(wsum, Wn.sum(axis=1)) and np.array_equal(wsum, pwsum)
        assert np.array_equal(sums, psums)
        j0 = 0
        for t, (v, dc, D, M) in enumerate(rows):
            want = [np.sum(Wn[0] * (v - Y[0]) ** 2)] + [np.sum(Wn[1 + k] * (D[d - 1] - Y[1 + k]) ** 2)
                                                          for k, d in enumerate(dirs)]
            assert max(want) < 2 ** 24
            assert np.array_equal(sums[t], np.asarray(want)), (dirs, t, sums[t], want)
            for j in range(len(dc)):
                wg = [np.sum(Wn[0] * 2 * (v - Y[0]) * dc[j])] + [
                    np.sum(Wn[1 + k] * 2 * (D[d - 1] - Y[1 + k]) * M[d - 1][j]) for k, d in enumerate(dirs)]
                big = [np.sum(Wn[0] * np.abs(2 * (v - Y[0]) * dc[j]))] + [
                    np.sum(Wn[1 + k] * np.abs(2 * (D[d - 1] - Y[1 + k]) * M[d - 1][j])) for k, d in enumerate(dirs)]
                assert max(big) < 2 ** 24
                assert np.array_equal(grads[j0 + j], np.asarray(wg)), (dirs, t, j, grads[j0 + j], wg)
            j0 += len(dc)
        assert j0 == grads.shape[0]


# ---- 2. fixture trees ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    with np.load(GOLDEN / "deriv_grad_cases.npz") as z:
        fx = {k: z[k] for k in z.files}
    for v in fx.values():
        v.setflags(write=False)
    return fx


@functools.lru_cache(maxsize=None)
def generator():
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_deriv_grad_golden", GOLDEN / "make_deriv_grad_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("T", [np.float32, np.float64], **TIDS)
def test_fixture_trees(gpu_ctx, T):
    """Every channel's gradient sum against mpmath's per-row ∂ŷ/∂x and ∂²ŷ/∂x∂c (module docstring),
    and the loss sums against srhip_eval_loss_deriv's bit for bit. No tree is skipped."""
    fx = cases()
    gen = generator()
    tn = "f32" if T == np.float32 else "f64"
    o, trees = gen.options(), gen.trees()
    assert len(trees) == int(fx["ntrees"]) == 28
    X = fx["X"].astype(T)
    assert np.array_equal(X.astype(np.float64), fx["X"]) and X.shape == (4, 293)  # the operands are Float32 values
    dirs = [int(d) for d in fx["dirs"]]
    Y, W = make_targets(X, dirs, T, 203)
    (sums, grads, wsum, ok), (psums, pwsum, pok) = run_grad(gpu_ctx, trees, o, X, Y, W, dirs, T)
    assert gpu_ctx.last_kernel_name() == kname(T)
    assert ok.all() and pok.all()
    assert np.array_equal(sums, psums) and np.array_equal(wsum, pwsum)
    coff = fx["const_off"]
    assert grads.shape == (coff[-1], 1 + len(dirs))
    assert (np.diff(coff) > 2).sum() >= 6  # trees with more constants than GC
    sv, sdc, sdx, sdxc = (gen.decode(fx[f"{tn}/{k}"]) for k in ("sv", "sdc", "sdx", "sdxc"))
    rt = RTOL[T]

    def delta(v, s):
        return rt * np.abs(v) + rt + 4 * s

    Wd, Yd = W.astype(np.float64), Y.astype(np.float64)
    worst = 0.0
    for t in range(len(trees)):
        for j in range(coff[t], coff[t + 1]):
            for c in range(1 + len(dirs)):
                if c == 0:
                    d, sd, m, sm = fx["v"][t], sv[t], fx["dc"][j], sdc[j]
                else:
                    d, sd, m, sm = fx["dx"][t, c - 1], sdx[t, c - 1], fx["dxc"][j, c - 1], sdxc[j, c - 1]
                r = d - Yd[c]
                ref = np.sum(Wd[c] * 2 * r * m)
                dd, dm = delta(d, sd), delta(m, sm)
                tol = np.sum(Wd[c] * (2 * dd * (np.abs(m) + dm) + 2 * np.abs(r) * dm)) + BAR[T] * np.sum(
                    Wd[c] * np.abs(2 * r * m))
                got = grads[j, c]
                print(f"tree {t} const {j} channel {c}: got {got!r} ref {ref!r} err {abs(got - ref):.3e} tol {tol:.3e}")
                worst = max(worst, abs(got - ref) / tol)
                assert abs(got - ref) <= tol, (t, j, c, got, ref, tol)
    print("worst error / bound", worst)


# ---- 3. group permutations ---------------------------------------------------------------------
def many_constant_trees(o):
    """Trees of 1, 3, 4 and 5 constants (more than GC in either variant), each constant in its own term."""
    B, U = o.make_binary, o.make_unary

    def term(c, f, g):
        return B("*", Node(val=c), B("*", Node(f"x{f}"), U("cos", Node(f"x{g}"))))

    cs = [0.75, -1.25, 0.5, 1.5, -0.625]
    out = []
    for nc in (1, 3, 4, 5):
        t = term(cs[0], 1, 2)
        for k in range(1, nc):
            t = B("+", t, term(cs[k], 1 + k % 4, 1 + (k + 2) % 4))
        out.append(U("exp", B("*", Node(val=0.25), t)) if nc == 3 else t)
    return out


def permuted_constants_tree(o, perm):
    """Σ_k c_perm[k]·x·cos(x): the same terms in the same order, the constants met in another order."""
    B, U = o.make_binary, o.make_unary
    cs = [0.75, -1.25, 0.5, 1.5, -0.625]
    t = None
    for k in perm:
        term = B("*", B("*", Node(f"x{1 + k % 4}"), U("cos", Node(f"x{1 + (k + 2) % 4}"))), Node(val=cs[k]))
        t = term if t is None else B("+", t, term)
    return t


@pytest.mark.parametrize("T", [np.float32, np.float64], **TIDS)
def test_direction_permutation(gpu_ctx, T):
    """A channel's sums do not depend on its place in the direction list: [d1, d2, d3] against a
    permutation, loss and gradient sums bit for bit (both lists run the R = 2 Float32 variant)."""
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    trees = many_constant_trees(o)
    X = np.random.default_rng(211).standard_normal((4, 300)).astype(T)
    d = [2, 4, 1]
    Y, W = make_targets(X, d, T, 212)
    (a, ga, wa, oka), _ = run_grad(gpu_ctx, trees, o, X, Y, W, d, T)
    perm = [2, 0, 1]
    cols = [0] + [1 + k for k in perm]
    (b, gb, wb, okb), _ = run_grad(gpu_ctx, trees, o, X, Y[cols], W[cols], [d[k] for k in perm], T)
    assert oka.all() and okb.all() and np.isfinite(ga).all()
    assert np.array_equal(a[:, cols], b) and np.array_equal(ga[:, cols], gb) and np.array_equal(wa[cols], wb)


@pytest.mark.parametrize("T", [np.float32, np.float64], **TIDS)
def test_constant_group_permutation(gpu_ctx, T):
    """A constant's gradient sums do not depend on its index, that is on its constant group and
    its slot in it: the 5-term sum with its terms in another order gives, per constant, sums that
    differ only through the value's own rounding — so the terms are chosen to make ŷ exact
    (each term c·x·cos(x') is evaluated alone, and the test compares the per-constant sums of
    single-term trees, whose value never depends on the order): constant k as tree k's only
    constant against the same constant as one of five in a tree whose other constants are 0."""
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    B, U = o.make_binary, o.make_unary
    cs = [0.75, -1.25, 0.5, 1.5, -0.625]
    X = np.random.default_rng(213).standard_normal((4, 300)).astype(T)
    d = [1, 3]
    Y, W = make_targets(X, d, T, 214)

    def term(c, k):
        return B("*", B("*", Node(f"x{1 + k % 4}"), U("cos", Node(f"x{1 + (k + 2) % 4}"))), Node(val=c))

    def five(k_live, order):
        """Σ over `order` of terms whose constant is 0 except term k_live: ŷ is that term exactly
        (x + 0 == x and 0·finite == ±0 add nothing), whatever the order."""
        t = None
        for k in order:
            tm = term(cs[k] if k == k_live else 0.0, k)
            t = tm if t is None else B("+", t, tm)
        return t

    orders = ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1])
    for k in range(5):
        (s1, g1, _, ok1), _ = run_grad(gpu_ctx, [term(cs[k], k)], o, X, Y, W, d, T)
        for order in orders:
            (s5, g5, _, ok5), _ = run_grad(gpu_ctx, [five(k, order)], o, X, Y, W, d, T)
            assert ok1.all() and ok5.all()
            assert np.array_equal(s1, s5), (k, order)
            assert np.array_equal(g1[0], g5[order.index(k)]), (k, order, g1[0], g5[order.index(k)])


# ---- 4. variants and losses --------------------------------------------------------------------
@pytest.mark.parametrize("T", [np.float32, np.float64], **TIDS)
def test_deep_variant_matches_central_differences(gpu_ctx, T):
    """A depth-6 tree runs the 16-slot variant. Its gradient sums against central differences of
    srhip_eval_loss_deriv's own sums in Float64 (h = 1e-6: truncation h² f''' ~ 1e-12 relative,
    rounding 1e-16 / h = 1e-10, so rtol 1e-7 with the sums' scale as atol); Float32 against the
    Float64 gradient with the sum bar of the loss-gradient slices (RTOL of the derivative tests)."""
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    trees = [deep_tree(o), o.make_binary("*", Node(val=1.5), o.make_binary("*", Node("x1"), Node("x3")))]
    X = (np.random.default_rng(97).random((4, 300)) + 0.5)
    dirs = [3, 1]
    Y, W = make_targets(X, dirs, np.float64, 98)
    ds64 = MultiDeviceDataset(gpu_ctx, X, Y, W)
    flat = srhip.flatten(trees, o, dtype=np.float64)
    prog = Program(gpu_ctx, flat, np.float64, interpreted=True)
    d0 = [d - 1 for d in dirs]
    sums, g64, wsum, ok = prog.eval_loss_grad_deriv(ds64, L2, d0)
    assert prog.pass_info()["grad_items"][3] >= 1 and ok.all()
    assert gpu_ctx.last_kernel_name() == kname(np.float64)
    nc = int(flat.const_off[-1])
    assert nc >= 10
    h = 1e-6
    fd = np.zeros_like(g64)
    base = np.asarray(flat.consts, dtype=np.float64).copy()
    for j in range(nc):
        tj = int(np.searchsorted(flat.const_off, j, side="right") - 1)
        vals = []
        for s in (+1, -1):
            c = base.copy()
            c[j] += s * h
            prog.set_constants(c)
            vals.append(prog.eval_loss_deriv(ds64, L2, d0)[0][tj])
        fd[j] = (vals[0] - vals[1]) / (2 * h)
    scale = np.abs(sums).max()
    assert np.allclose(g64, fd, rtol=1e-7, atol=1e-7 * scale), np.abs(g64 - fd).max()
    if T == np.float32:
        ds32 = MultiDeviceDataset(gpu_ctx, X.astype(T), Y.astype(T), W.astype(T))
        p32 = Program(gpu_ctx, srhip.flatten(trees, o, dtype=T), T, interpreted=True)
        s32, g32, _, ok32 = p32.eval_loss_grad_deriv(ds32, L2, d0)
        assert gpu_ctx.last_kernel_name() == kname(T) and ok32.all()
        assert np.allclose(g32, g64, rtol=RTOL[T], atol=RTOL[T] * scale)


@pytest.mark.parametrize("T", [np.float32, np.float64], **TIDS)
@pytest.mark.parametrize("loss", [(L1, 0.0), (HUBER, 1.0)], ids=["L1", "Huber"])
def test_l1_and_huber(gpu_ctx, T, loss):
    """ℓ' of another table loss multiplies the mixed partial. On the exact trees every term is a
    small integer or half-integer, so the sums are exact: L1's ℓ' = sign(r), Huber(1)'s r inside
    |r| <= 1 and sign(r) outside."""
    kind, param = loss
    o = srhip.Options(binary_operators=["+", "-", "*"], unary_operators=[])
    rng = np.random.default_rng(7)
    n = 300
    X = rng.integers(1, 4, (4, n)).astype(np.float64)
    dirs = [2, 1]
    Y = rng.integers(-3, 4, (3, n)).astype(np.float64)
    Y[0] += 20
    (sums, grads, wsum, ok), (psums, _, _) = run_grad(gpu_ctx, exact_trees(o), o, X.astype(T), Y.astype(T), None, dirs, T,
                                                       kind, [param])
    assert ok.all() and np.array_equal(sums, psums)

    def dl(r):
        return np.sign(r) if kind == L1 else np.where(np.abs(r) <= param, r, param * np.sign(r))

    j0 = 0
    for t, (v, dc, D, M) in enumerate(exact_rows(X)):
        for j in range(len(dc)):
            want = [np.sum(dl(v - Y[0]) * dc[j])] + [np.sum(dl(D[d - 1] - Y[1 + k]) * M[d - 1][j]) for k, d in enumerate(dirs)]
            assert np.array_equal(grads[j0 + j], np.asarray(want)), (t, j, grads[j0 + j], want)
        j0 += len(dc)


@pytest.mark.parametrize("T", [np.float32, np.float64], **TIDS)
def test_non_finite_rule(gpu_ctx, T):
    """c1·safe_sqrt(x1) at x1 = 0: the value is finite, the derivative and the mixed partial are
    not: ok = 1, channel 0's loss sum finite, channel 1's loss and gradient sums not. A tree that fails
    (log of a negative row) has ok = 0 and NaN rows in both outputs."""
    o = srhip.Options(binary_operators=["+", "*"], unary_operators=["safe_sqrt", "safe_log"])
    B, U = o.make_binary, o.make_unary
    trees = [B("*", Node(val=1.5), U("safe_sqrt", Node("x1"))), B("*", Node(val=1.5), U("safe_log", Node("x2")))]
    X = np.zeros((2, 300), dtype=T)
    X[0, 1:] = np.linspace(0.5, 2.0, 299)
    X[1] = -1.0
    Y = np.ones((2, 300), dtype=T)
    (sums, grads, wsum, ok), (psums, _, pok) = run_grad(gpu_ctx, trees, o, X, Y, None, [1], T)
    assert list(ok) == [True, False] and list(pok) == [True, False]
    assert np.isfinite(sums[0, 0]) and not np.isfinite(sums[0, 1])
    assert not np.isfinite(grads[0, 1])  # (channel 0's is the first-order rule's: 0 · Inf inside the root)
    assert np.isnan(sums[1]).all() and np.isnan(grads[1]).all()
    assert np.array_equal(sums, psums, equal_nan=True)
    oo = srhip.Options(binary_operators=["+", "*"], unary_operators=["safe_sqrt", "safe_log"],
                       loss_function=srhip.DerivativeObjective([1.0, 1.0]))
    dds = srhip.DerivativeDataset(X, Y[0], Y[1:], [1])
    v, g, vok = srhip.eval_deriv_loss_grad_batch(trees, dds, oo)
    assert (v == np.inf).all() and list(vok) == [True, False] and np.isnan(g[1])


# ---- 5. refusals -----------------------------------------------------------------------------------
def test_refusals_before_any_launch():
    """Each refusal returns its code, leaves the outputs untouched and launches nothing (a context
    of its own, whose launch count stays 0): srhip_eval_loss_deriv's table, and the plans that would
    run wide (no tile of 330 features fits LDS; SRHIP_WIDE=1 is read per call)."""
    import os

    T = np.float32
    ctx = srhip.Context(0)
    objs = []
    try:
        o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
        X = np.random.default_rng(1).standard_normal((4, 64)).astype(T)
        ds = MultiDeviceDataset(ctx, X, np.zeros((3, 64), dtype=T))
        tree = o.make_binary("*", Node(val=2.0), o.make_binary("*", Node("x1"), Node("x2")))
        flat = srhip.flatten([tree], o, dtype=T)
        prog = Program(ctx, flat, T, interpreted=True)
        xo = EO.options(("dbl",))
        xprog = Program(ctx, srhip.flatten([xo.make_unary("dbl", Node("x1"))], xo, dtype=T), T, interpreted=True)
        Xw = np.random.default_rng(2).standard_normal((330, 64)).astype(T)
        dsw = MultiDeviceDataset(ctx, Xw, np.zeros((3, 64), dtype=T))
        objs += [prog, xprog, ds, dsw]
        L = _lib.lib()
        huber = np.asarray([1.0])

        def call(p, kind, dirs, ndir=None, dataset=ds, null_dir=False, params=huber):
            d = np.asarray(dirs, dtype=np.int32)
            sums, grads, wsum = np.full(8, -7.0), np.full(8, -7.0), np.full(8, -7.0)
            ok = np.full(4, 9, dtype=np.uint8)
            rc = L.srhip_eval_loss_grad_deriv(dataset.handle, p.handle, kind, params.ctypes.data,
                                              None if null_dir else d.ctypes.data, len(d) if ndir is None else ndir,
                                              sums.ctypes.data, grads.ctypes.data, wsum.ctypes.data, ok.ctypes.data)
            assert (sums == -7.0).all() and (grads == -7.0).all() and (wsum == -7.0).all() and (ok == 9).all()
            return rc

        def mixed(p, dirs, dataset=ds):
            d = np.asarray(dirs, dtype=np.int32)
            der, mix = np.full((4, 64), -7.0, dtype=T), np.full((4, 64), -7.0, dtype=T)
            ok = np.full(4, 9, dtype=np.uint8)
            rc = L.srhip_eval_mixed_tree_array(dataset.handle, p.handle, d.ctypes.data, len(d), der.ctypes.data,
                                               mix.ctypes.data, ok.ctypes.data)
            assert (der == -7.0).all() and (mix == -7.0).all() and (ok == 9).all()
            return rc

        def optimise(dirs, coef, dataset=ds, kind=L2):
            d = np.asarray(dirs, dtype=np.int32)
            cf = np.asarray(coef, dtype=np.float64)
            noise = np.zeros(2)
            opts = _lib.ConstOptOptions(0, 8, 2, kind, huber.ctypes.data_as(C.POINTER(C.c_double)),
                                        noise.ctypes.data_as(C.POINTER(C.c_double)), 0)
            consts = np.ascontiguousarray(flat.consts, dtype=T)
            tr = srhip.engine._trees_struct(flat, consts)
            oc, ol, on = np.full(2, -7.0, dtype=T), np.full(2, -7.0), np.full(2, -7.0)
            ok = np.full(2, 9, dtype=np.uint8)
            rc = L.srhip_optimize_constants_deriv(ctx.handle, dataset.handle, C.byref(tr), C.byref(opts), d.ctypes.data,
                                                  len(d), cf.ctypes.data if len(cf) else None, oc.ctypes.data,
                                                  ol.ctypes.data, ok.ctypes.data, on.ctypes.data)
            assert (oc == -7.0).all() and (ol == -7.0).all() and (on == -7.0).all() and (ok == 9).all()
            return rc

        INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
        assert call(prog, L2, [0, 1], null_dir=True) == INV
        assert call(prog, L2, [], ndir=0) == INV
        assert call(prog, L2, list(range(16)), ndir=16) == INV
        assert call(prog, L2, [0]) == INV  # 3 columns, 1 direction
        assert call(prog, L2, [0, 4]) == INV
        assert call(prog, L2, [-1, 0]) == INV
        assert call(prog, L2, [1, 1]) == INV
        assert call(prog, K.MARGIN_LOSS_BEGIN, [0, 1]) == INV
        assert call(prog, EL.expr_loss("SQ").kind, [0, 1]) == UNS
        assert call(xprog, L2, [0, 1]) == UNS
        progw = Program(ctx, srhip.flatten([o.make_binary("*", Node(val=2.0), Node("x330"))], o, dtype=T), T,
                        interpreted=True)
        objs.insert(0, progw)
        assert call(progw, L2, [0, 329], dataset=dsw) == UNS  # plans wide
        assert b"wide" in L.srhip_last_error()
        os.environ["SRHIP_WIDE"] = "1"
        try:
            assert call(prog, L2, [0, 1]) == UNS
            assert mixed(prog, [0, 1]) == UNS
            assert optimise([0, 1], [1.0, 1.0, 1.0]) == UNS
        finally:
            del os.environ["SRHIP_WIDE"]
        assert mixed(prog, [0, 4]) == INV and mixed(prog, [1, 1]) == INV and mixed(xprog, [0]) == UNS
        assert mixed(progw, [0], dataset=dsw) == UNS
        assert optimise([0], [1.0, 1.0]) == INV  # 3 columns, 1 direction
        assert optimise([0, 1], []) == INV  # null coef
        assert optimise([0, 1], [1.0, np.nan, 1.0]) == INV
        assert optimise([0, 1], [1.0, 1.0, 1.0], kind=EL.expr_loss("SQ").kind) == UNS
        assert ctx.last_kernel_time()[1] == 0
        sums, grads, wsum, ok = prog.eval_loss_grad_deriv(ds, L2, [0, 1])
        assert ctx.last_kernel_time()[1] >= 1 and ok.all()
    finally:
        for obj in objs:  # destroyed now, before their context is closed
            obj.__del__()
        ctx.close()


# ---- 6. the optimiser ----------------------------------------------------------------------------
class DerivEvaluator:
    """The callback evaluator of srhip_optimize_constants_cb: gradient phases through
    eval_loss_grad_deriv, loss-only phases through eval_loss_deriv, combined as the C entry
    documents it (float64, channel order)."""

    def __init__(self, ctx, ds, cands, o, T, dirs, coef):
        self.ds, self.dirs, self.coef, self.T = ds, [d - 1 for d in dirs], coef, T
        self.flat = srhip.flatten(cands, o, dtype=T)
        self.prog = Program(ctx, self.flat, T, interpreted=True)

    def _combine(self, a, wsum):
        v = np.zeros(a.shape[0])
        for c in range(a.shape[1]):
            v = v + self.coef[c] * a[:, c] / wsum[c]
        return v

    def loss_only(self, x):
        self.prog.set_constants(np.asarray(x, dtype=self.T))
        sums, wsum, ok = self.prog.eval_loss_deriv(self.ds, L2, self.dirs)
        with np.errstate(all="ignore"):
            f = self._combine(sums, wsum)
        return np.where(ok & np.isfinite(f), f, np.inf)

    def loss_grad(self, x):
        self.prog.set_constants(np.asarray(x, dtype=self.T))
        sums, grads, wsum, ok = self.prog.eval_loss_grad_deriv(self.ds, L2, self.dirs)
        with np.errstate(all="ignore"):
            f = self._combine(sums, wsum)
            g = self._combine(grads, wsum)
        g[np.repeat(~ok, np.diff(self.flat.const_off))] = np.nan
        return np.where(ok & np.isfinite(f), f, np.inf), g


@pytest.mark.parametrize("T", [np.float32, np.float64], **TIDS)
@pytest.mark.parametrize("algorithm", ["BFGS", "NelderMead"])
def test_optimiser_plumbing(gpu_ctx, T, algorithm):
    """srhip_optimize_constants_deriv against srhip_optimize_constants_cb driven by a callback that
    calls eval_loss_grad_deriv / eval_loss_deriv, the same start noise: constants, losses, converged
    flags and num_evals identical."""
    from srhip.constant_optimization import _Callback, start_noise, ALGORITHMS

    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"],
                      optimizer_algorithm=algorithm)
    trees = many_constant_trees(o) + [Node("x1")]
    X = np.random.default_rng(221).standard_normal((4, 300)).astype(T)
    dirs = [1, 3]
    Y, W = make_targets(X, dirs, T, 222)
    coef = np.asarray([1.0, 0.5, 0.25])
    dds = srhip.DerivativeDataset(X, Y[0], Y[1:], dirs, W)
    oo = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"],
                       optimizer_algorithm=algorithm, loss_function=srhip.DerivativeObjective(coef))
    flat = srhip.flatten(trees, o, dtype=T)
    noise = start_noise(flat, 2, np.random.default_rng(223))
    a = [t.copy() for t in trees]
    ra = srhip.optimize_constants_deriv_batch(dds, a, oo, noise=noise)
    # the same run through the callback entry
    dev = dds.multi.device(None)
    b = [t.copy() for t in trees]
    cb = _Callback(b, lambda cands: DerivEvaluator(dev.ctx, dev, cands, o, T, dirs, coef))
    par = None
    opts = _lib.ConstOptOptions(ALGORITHMS[algorithm], 8, 2, L2, par, noise.ctypes.data_as(C.POINTER(C.c_double)), 0)
    consts = np.ascontiguousarray(flat.consts, dtype=T)
    tr = srhip.engine._trees_struct(flat, consts)
    nt = len(trees)
    out_c, out_l = np.zeros(consts.size, dtype=T), np.zeros(nt)
    out_k, out_n = np.zeros(nt, dtype=np.uint8), np.zeros(nt)
    rc = _lib.lib().srhip_optimize_constants_cb(C.byref(tr), 0 if T == np.float32 else 1, C.byref(opts), cb.fn, None,
                                                *[x.ctypes.data_as(C.c_void_p) for x in (out_c, out_l, out_k, out_n)])
    if cb.error is not None:
        raise cb.error
    _lib.check(rc)
    assert np.array_equal(ra.converged, out_k.astype(bool))
    assert np.array_equal(ra.num_evals, out_n)
    assert np.array_equal(ra.losses, out_l)
    got = srhip.flatten(a, o, dtype=T).consts
    want = np.where(np.repeat(out_k.astype(bool), np.diff(flat.const_off)), out_c, consts)
    assert np.array_equal(np.asarray(got, dtype=T), want)
    assert ra.num_evals[:-1].min() > 0 and ra.converged[:-1].any()
    prof = srhip.constant_optimization.last_profile()
    print("profile", prof)


def test_end_to_end_fits_the_derivative_channel(gpu_ctx):
    """Data from 1.5·x1² − 0.5·x1; tree c1·x1·x1 + c2·x1 started at (1, 1); coefficients (0, 1), so
    only the derivative channel can move the constants. The optimised objective falls below 1e-8 of
    its start in Float64 and the tree is marked converged."""
    T = np.float64
    obj = srhip.DerivativeObjective([0.0, 1.0])
    o = srhip.Options(binary_operators=["+", "-", "*"], unary_operators=[], loss_function=obj)
    B = o.make_binary
    tree = B("+", B("*", B("*", Node(val=1.0), Node("x1")), Node("x1")), B("*", Node(val=1.0), Node("x1")))
    rng = np.random.default_rng(231)
    X = rng.uniform(-2, 2, (2, 300)).astype(T)
    y = 1.5 * X[0] ** 2 - 0.5 * X[0]
    g = (3.0 * X[0] - 0.5)[None, :]
    dds = srhip.DerivativeDataset(X, y, g, [1])
    start, _, ok0 = srhip.eval_deriv_loss_grad_batch([tree], dds, o)
    assert ok0.all() and start[0] > 0.1
    r = srhip.optimize_constants_deriv_batch(dds, [tree], o, rng=np.random.default_rng(232))
    assert r.converged[0]
    print("objective", start[0], "->", r.losses[0], "constants", srhip.flatten([tree], o, dtype=T).consts)
    assert r.losses[0] < 1e-8 * start[0]
    prof = srhip.constant_optimization.last_profile()
    assert prof["n_grad"] >= 1 and prof["n_loss"] >= 1
