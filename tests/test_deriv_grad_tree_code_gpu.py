"""The objective's one-pass gradient tree code: srhip_eval_objective_grad_deriv
on a SRHIP_PROGRAM_DERIV_GRAD_TREE_CODE program against exact integer sums and the mpmath fixture
of tests/test_deriv_grad_gpu.py, its fallbacks and refusals, and the optimiser running on it.

Fixture bound: the reference is Σ_c q_c·ref_c and the bound Σ_c |q_c|·tol_c, with ref_c and tol_c
the per-channel reference and bound of tests/test_deriv_grad_gpu.py (its docstring) at RTOL / BAR
for Float32; q_c's one rounding to float (2^-24 of each term) lies inside BAR = 1e-5 of Σ|terms|.
Fallback equality: the engine rounds each product q_c·column_c and adds them in channel order in
float64 (srhip.h), which the test repeats, so the comparison is bit for bit."""
import numpy as np
import pytest

import srhip
from srhip import Node, _lib
from srhip import constants as K
from srhip.engine import MultiDeviceDataset, Program
from test_deriv_grad_gpu import cases, generator
from test_deriv_loss_gpu import BAR, RTOL, make_targets

pytestmark = pytest.mark.gpu

L2, L1 = K.LOSS["L2"], K.LOSS["L1"]
T = np.float32
C1, C2 = 2.0, 3.0


def exact_trees(o, c1=C1, c2=C2):
    """test_deriv_grad_gpu.exact_trees, and a tree without the direction features' subtree."""
    B = o.make_binary
    x1, x2 = (lambda: Node("x1")), (lambda: Node("x2"))
    return [B("+", B("*", B("*", Node(val=c1), x1()), x1()), B("*", B("*", Node(val=c2), x1()), x2())),
            B("-", B("*", Node(val=c1), x1()), B("*", B("*", Node(val=c2), x2()), x2())),
            B("*", Node(val=c1), x1()),
            Node(val=c1),
            B("*", Node(val=c1), B("*", Node("x4"), Node("x4")))]


def exact_rows(X, c1=C1, c2=C2):
    """Per tree (ŷ, ∂ŷ/∂c [nc], ∂ŷ/∂x [3], ∂²ŷ/∂x∂c [3][nc]) in exact integer arithmetic."""
    x1, x2, x4 = X[0], X[1], X[3]
    z, one = np.zeros_like(x1), np.ones_like(x1)
    return [(c1 * x1 * x1 + c2 * x1 * x2, [x1 * x1, x1 * x2], [2 * c1 * x1 + c2 * x2, c2 * x1, z],
             [[2 * x1, x2], [z, x1], [z, z]]),
            (c1 * x1 - c2 * x2 * x2, [x1, -x2 * x2], [c1 * one, -2 * c2 * x2, z], [[one, z], [z, -2 * x2], [z, z]]),
            (c1 * x1, [x1], [c1 * one, z, z], [[one], [z], [z]]),
            (c1 * one, [one], [z, z, z], [[z], [z], [z]]),
            (c1 * x4 * x4, [x4 * x4], [z, z, z], [[z], [z], [z]])]


def check_exact(ctx, prog, plain, ds, X, Y, W, dirs, kind, c1=C1, c2=C2):
    d0 = [d - 1 for d in dirs]
    Wn = np.ones_like(Y) if W is None else W
    coef = Wn.sum(axis=1)  # q_c = 1 exactly
    sums, grad, wsum, ok = prog.eval_objective_grad_deriv(ds, kind, d0, coef)
    assert ctx.last_kernel_name() == ("sr_jit_deriv_grad" if W is None else "sr_jit_deriv_grad_w")
    assert ctx.last_tree_code() == 5
    nrg = ctx.last_loss_launch()["nrg"]
    psums, _, pok = plain.eval_loss_deriv(ds, kind, d0)
    assert ok.all() and pok.all() and np.array_equal(wsum, coef)
    assert np.array_equal(sums, psums)
    dl = (lambda r: 2 * r) if kind == L2 else np.sign
    j0, total = 0, 0.0
    for v, dc, D, M in exact_rows(X, c1, c2):
        for j in range(len(dc)):
            terms = [Wn[0] * dl(v - Y[0]) * dc[j]] + [Wn[1 + k] * dl(D[d - 1] - Y[1 + k]) * M[d - 1][j]
                                                     for k, d in enumerate(dirs)]
            total = max(total, sum(np.abs(t).sum() for t in terms))
            assert grad[j0 + j] == sum(t.sum() for t in terms), (dirs, j0 + j, grad[j0 + j])
        j0 += len(dc)
    assert j0 == grad.shape[0] and total < 2 ** 24
    return nrg


@pytest.mark.parametrize("kind", [L2, L1], ids=["L2", "L1"])
@pytest.mark.parametrize("n", [300, 2049])
@pytest.mark.parametrize("weighted", [False, True])
def test_exact_integer_cases(gpu_ctx, n, weighted, kind):
    """Small-integer data and q_c = 1: out_grad equals numpy's float64 Σ_c Σ_i w·ℓ'(r)·m bit for
    bit, the loss sums equal the dv tree code's, every tree compiles."""
    o = srhip.Options(binary_operators=["+", "-", "*"], unary_operators=[])
    rng = np.random.default_rng(5)
    X = rng.integers(1, 4, (4, n)).astype(np.float64)
    flat = srhip.flatten(exact_trees(o), o, dtype=T)
    prog = Program(gpu_ctx, flat, T, interpreted=True, deriv_grad_tree_code=True)
    plain = Program(gpu_ctx, flat, T, interpreted=True, deriv_tree_code=True)
    for dirs in ([1], [2, 1], [1, 2, 3]):
        Y = rng.integers(-3, 4, (1 + len(dirs), n)).astype(np.float64)
        Y[0] += 20
        if kind == L1:
            Y += 0.5  # no residual is 0
        W = rng.integers(1, 3, (1 + len(dirs), n)).astype(np.float64) if weighted else None
        ds = MultiDeviceDataset(gpu_ctx, X.astype(T), Y.astype(T), None if W is None else W.astype(T))
        nrg = check_exact(gpu_ctx, prog, plain, ds, X, Y, W, dirs, kind)
        assert nrg > 1 or n == 300
    # 3. set_constants: the same module, other small integers
    before = prog.update_stats()["rebuilt"]
    for p in (prog, plain):
        p.set_constants(np.asarray([3, 1, 3, 1, 3, 3, 3], dtype=T))
    assert prog.update_stats()["rebuilt"] == before
    check_exact(gpu_ctx, prog, plain, ds, X, Y, W, [1, 2, 3], kind, 3.0, 1.0)


def test_fixture_trees(gpu_ctx):
    """28 fixture trees, unequal coefficients, against mpmath (module docstring). Trees the code
    generator refuses run interpreted in the same call; none is skipped."""
    fx, gen = cases(), generator()
    o, trees = gen.options(), gen.trees()
    X = fx["X"].astype(T)
    dirs = [int(d) for d in fx["dirs"]]
    Y, W = make_targets(X, dirs, T, 203)
    coef = np.asarray([1.0, 0.5, 2.0, 0.25, 1.5][:1 + len(dirs)])
    ds = MultiDeviceDataset(gpu_ctx, X, Y, W)
    prog = Program(gpu_ctx, srhip.flatten(trees, o, dtype=T), T, interpreted=True, deriv_grad_tree_code=True)
    sums, grad, wsum, ok = prog.eval_objective_grad_deriv(ds, L2, [d - 1 for d in dirs], coef)
    ncomp = gpu_ctx.last_tree_code()
    print("compiled", ncomp, "of", len(trees))
    # the mode takes + - * / cos exp safe_sqrt safe_log of the fixture's operators: every tree but
    # the one with safe_pow and the one with tanh (these two run interpreted in the same call)
    assert ok.all() and ncomp == len(trees) - 2
    # the loss sums are the dv tree code's bit for bit (cos above direction leaves included); the safe_pow
    # tree is left out: it is tree code there and interpreted here
    psums, _, pok = Program(gpu_ctx, srhip.flatten(trees, o, dtype=T), T, interpreted=True,
                            deriv_tree_code=True).eval_loss_deriv(ds, L2, [d - 1 for d in dirs])
    same = [t for t in range(len(trees)) if "safe_pow" not in srhip.string_tree(trees[t], o)]
    assert len(same) == len(trees) - 1 and pok.all() and np.array_equal(sums[same], psums[same])
    q = coef / wsum
    coff = fx["const_off"]
    sv, sdc, sdx, sdxc = (gen.decode(fx[f"f32/{k}"]) for k in ("sv", "sdc", "sdx", "sdxc"))
    rt = RTOL[T]

    def delta(v, s):
        return rt * np.abs(v) + rt + 4 * s

    Wd, Yd = W.astype(np.float64), Y.astype(np.float64)
    worst = 0.0
    for t in range(len(trees)):
        for j in range(coff[t], coff[t + 1]):
            ref = tol = 0.0
            for c in range(1 + len(dirs)):
                if c == 0:
                    d, sd, m, sm = fx["v"][t], sv[t], fx["dc"][j], sdc[j]
                else:
                    d, sd, m, sm = fx["dx"][t, c - 1], sdx[t, c - 1], fx["dxc"][j, c - 1], sdxc[j, c - 1]
                r = d - Yd[c]
                dd, dm = delta(d, sd), delta(m, sm)
                ref += q[c] * np.sum(Wd[c] * 2 * r * m)
                tol += abs(q[c]) * (np.sum(Wd[c] * (2 * dd * (np.abs(m) + dm) + 2 * np.abs(r) * dm)) +
                                    BAR[T] * np.sum(Wd[c] * np.abs(2 * r * m)))
            print(f"tree {t} const {j}: got {grad[j]!r} ref {ref!r} err {abs(grad[j] - ref):.3e} tol {tol:.3e}")
            worst = max(worst, abs(grad[j] - ref) / tol)
    print("worst error / bound", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("case", ["ndir5", "float64"])
def test_fallbacks(gpu_ctx, case):
    """Past a limit the call is the interpreter's columns combined with q_c (module docstring)."""
    Tc = np.float64 if case == "float64" else np.float32
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    B, U = o.make_binary, o.make_unary
    trees = [B("*", Node(val=1.5), B("*", Node("x1"), U("cos", B("*", Node(val=0.5), Node("x2"))))), B("+", Node(val=2.0), Node("x3"))]
    dirs = [0, 1, 2, 3, 4] if case == "ndir5" else [1, 0]
    X = np.random.default_rng(7).standard_normal((5, 300)).astype(Tc)
    Y, W = make_targets(X, dirs, Tc, 8)
    ds = MultiDeviceDataset(gpu_ctx, X, Y, W)
    prog = Program(gpu_ctx, srhip.flatten(trees, o, dtype=Tc), Tc, interpreted=True, deriv_grad_tree_code=True)
    coef = np.linspace(1.0, 2.0, 1 + len(dirs))
    sums, grad, wsum, ok = prog.eval_objective_grad_deriv(ds, L2, dirs, coef)
    assert gpu_ctx.last_tree_code() == 0
    csums, cols, cw, cok = prog.eval_loss_grad_deriv(ds, L2, dirs)
    assert np.array_equal(sums, csums) and np.array_equal(wsum, cw) and ok.all() and cok.all()
    q = coef / cw
    want = np.zeros(cols.shape[0])
    for c in range(1 + len(dirs)):
        want = want + q[c] * cols[:, c]
    assert np.array_equal(grad, want)


@pytest.mark.parametrize("case", ["coef", "wide"])
def test_refusals_leave_outputs_untouched(gpu_ctx, case):
    o = srhip.Options(binary_operators=["+", "*"], unary_operators=[])
    nf = 330 if case == "wide" else 4
    X = np.random.default_rng(1).standard_normal((nf, 64)).astype(T)
    ds = MultiDeviceDataset(gpu_ctx, X, np.zeros((2, 64), dtype=T))
    prog = Program(gpu_ctx, srhip.flatten([o.make_binary("*", Node(val=2.0), Node("x1"))], o, dtype=T), T,
                   interpreted=True, deriv_grad_tree_code=True)
    d = np.asarray([0], dtype=np.int32)
    coef = np.asarray([1.0, np.inf if case == "coef" else 1.0])
    outs = [np.full(4, -7.0) for _ in range(3)]
    okb = np.full(2, 9, dtype=np.uint8)
    rc = _lib.lib().srhip_eval_objective_grad_deriv(ds.handle, prog.handle, L2, None, d.ctypes.data, 1, coef.ctypes.data,
                                                    outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data,
                                                    okb.ctypes.data)
    assert rc != 0 and all((a == -7.0).all() for a in outs) and (okb == 9).all()


def test_optimiser_runs_on_the_tree_code(gpu_ctx):
    """test_deriv_grad_gpu's end-to-end fit (data from 1.5·x1² − 0.5·x1, coefficients (0, 1)) in
    Float32 with grad_tree_code=True: that test's recovery tolerance, and the new kernel's name."""
    obj = srhip.DerivativeObjective([0.0, 1.0], grad_tree_code=True)
    o = srhip.Options(binary_operators=["+", "-", "*"], unary_operators=[], loss_function=obj)
    B = o.make_binary
    tree = B("+", B("*", B("*", Node(val=1.0), Node("x1")), Node("x1")), B("*", Node(val=1.0), Node("x1")))
    rng = np.random.default_rng(231)
    X = rng.uniform(-2, 2, (2, 300)).astype(T)
    y = (1.5 * X[0].astype(np.float64) ** 2 - 0.5 * X[0]).astype(T)
    g = (3.0 * X[0].astype(np.float64) - 0.5).astype(T)[None, :]
    dds = srhip.DerivativeDataset(X, y, g, [1])
    start, g0, ok0 = srhip.eval_deriv_objective_grad_batch([tree], dds, o)
    ctx = dds.multi.device(None).ctx
    assert ctx.last_kernel_name() == "sr_jit_deriv_grad" and ctx.last_tree_code() == 1
    assert ok0.all() and start[0] > 0.1 and np.isfinite(g0).all()
    r = srhip.optimize_constants_deriv_batch(dds, [tree], o, rng=np.random.default_rng(232))
    print("objective", start[0], "->", r.losses[0], "constants", srhip.flatten([tree], o, dtype=T).consts)
    assert r.converged[0] and r.losses[0] < 1e-8 * start[0]
    prof = srhip.constant_optimization.last_profile()
    # every gradient call of the run itself ran the new tree code; its last call either tree code
    assert prof["n_loss"] >= 1 and prof["n_grad_tree_code"] == prof["n_grad"] >= 1
    assert ctx.last_kernel_name() in ("sr_jit_deriv", "sr_jit_deriv_grad") and ctx.last_tree_code() == 1
