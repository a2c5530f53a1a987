"""Derivative tree code on the GPU (SRHIP_PROGRAM_DERIV_TREE_CODE):
srhip_eval_loss_deriv as reverse-mode tree code ("sr_jit_deriv" / "sr_jit_deriv_w") against
the forward-mode interpreter of the same build and the Float64 oracle, with the references,
bounds and helpers of test_deriv_loss_gpu.py.

Row counts: 300 (a partial second 256-row tile) and 2049, the smallest count at which every
launch of test 1 has two row groups: the one-direction unweighted tile (y, 4 features, one
target: 6 KiB) gets 8 tiles = 2048 rows per workgroup within the 52 KiB tile budget, the other
variants 4 (checked through srhip_last_loss_launch)."""
import functools

import numpy as np
import pytest

import srhip
from srhip import Node
from srhip.engine import MultiDeviceDataset, Program
from test_deriv_loss_gpu import (HUBER, L1, L2, check_channels, exact_rows, exact_trees, make_targets, population,
                                 row_reference)

pytestmark = pytest.mark.gpu
T = np.float32


def run(ctx, trees, o, X, Y, W, dirs, kind=L2, params=None, tree_code=True):
    """(sums, ok, trees run as tree code, last kernel) of one eval_loss_deriv."""
    ds = MultiDeviceDataset(ctx, X, Y, W)
    prog = Program(ctx, srhip.flatten(trees, o, dtype=T), T, interpreted=True, deriv_tree_code=tree_code)
    sums, _, ok = prog.eval_loss_deriv(ds, kind, [d - 1 for d in dirs], params)
    return sums, ok, ctx.last_tree_code(), ctx.last_kernel_name()


def check_against_both(ctx, trees, o, X, refs, dirs, kind, param, seed, ncode, msg, singular=0):
    """Tree code vs the oracle (check_channels' bounds) and vs the interpreter (flags; channel 0 to 1e-5).
    A channel that is non-finite in both paths is the engine's non-finite-derivative case (a 0·∞ inside a
    rule the two share, §3.18's flag rule) where the oracle's is finite, and has no bound: at most `singular` of them, a property
    of the population stated by the caller. Every other channel, one where only the interpreter's forward
    mode is non-finite included, is held to the oracle."""
    Y, W = make_targets(X, dirs, T, seed)
    sums, ok, n, name = run(ctx, trees, o, X, Y, W, dirs, kind, [param])
    ref, rok, n0, _ = run(ctx, trees, o, X, Y, W, dirs, kind, [param], tree_code=False)
    assert (n, name, n0) == (ncode, "sr_jit_deriv_w", 0)
    assert np.array_equal(ok, rok) and np.isnan(sums[~ok]).all()
    np.testing.assert_allclose(sums[ok, 0], ref[ok, 0], rtol=1e-5, atol=0)
    nsing = 0
    for j, d in enumerate(dirs):
        with np.errstate(all="ignore"):  # (a row loss that overflows T is the oracle's own non-finite case)
            fin = np.asarray([np.isfinite((r[1][d - 1].astype(T) - Y[1 + j]) ** 2).all() for r in refs])
        both = ok & fin & ~np.isfinite(sums[:, 1 + j]) & ~np.isfinite(ref[:, 1 + j])
        nsing += int(both.sum())
        cols = [0, 1 + j]
        assert check_channels(sums[:, cols], ok & ~both, refs, [d], Y[cols], W[cols], T, kind, param,
                              msg=msg) == int((ok & ~both).sum())
    assert nsing <= singular, nsing
    return ok


@pytest.mark.parametrize("n", [300, 2049])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dirs", [[1], [2, 1], [1, 2, 3]], ids=str)
def test_exact_integer_cases(gpu_ctx, n, weighted, dirs):
    """Small-integer data, L2: every sum is an integer below 2^24, so tree code, interpreter and
    numpy agree bit for bit. x1*x1 (two occurrences of a direction), x1*x2 - x2*x2 (the sign
    flag), 2*x1 (a constant operand), a constant tree (no reverse code), direction 3 in no tree."""
    o = srhip.Options(binary_operators=["+", "-", "*"], unary_operators=[])
    rng = np.random.default_rng(5)
    X = rng.integers(1, 5, (4, n)).astype(T)
    Y = rng.integers(-3, 4, (1 + len(dirs), n)).astype(T)
    W = rng.integers(1, 4, (1 + len(dirs), n)).astype(T) if weighted else None
    sums, ok, ncode, name = run(gpu_ctx, exact_trees(o), o, X, Y, W, dirs)
    assert (ncode, name) == (4, "sr_jit_deriv_w" if weighted else "sr_jit_deriv")  # fails without the feature
    assert gpu_ctx.last_loss_launch()["nrg"] == (1 if n == 300 else 2 if dirs == [1] and not weighted else 3)
    ref, rok, n0, _ = run(gpu_ctx, exact_trees(o), o, X, Y, W, dirs, tree_code=False)
    assert n0 == 0 and ok.all() and rok.all()
    assert np.array_equal(sums, ref)
    Wn = np.ones_like(Y) if W is None else W
    for t, (v, D) in enumerate(exact_rows(X.astype(np.float64))):
        want = [np.sum(Wn[0] * (v - Y[0]) ** 2)] + [np.sum(Wn[1 + j] * (D[d - 1] - Y[1 + j]) ** 2) for j, d in enumerate(dirs)]
        assert np.array_equal(sums[t], np.asarray(want, dtype=np.float64)), (t, sums[t], want)


@pytest.mark.parametrize("dirs,kind,param", [([1], L2, 0.0), ([3, 1], L2, 0.0), ([1, 2, 3, 4], L2, 0.0),
                                             ([3, 1], L1, 0.0), ([3, 1], HUBER, 1.0)], ids=str)
def test_population_vs_oracle(gpu_ctx, dirs, kind, param):
    o, trees, X, refs = population(T)
    ok = check_against_both(gpu_ctx, trees, o, X, refs, dirs, kind, param, 93, 200, f"population {dirs} {kind}")
    assert ok.sum() >= 150


@functools.lru_cache(maxsize=None)
def routine_population():
    o = srhip.Options(binary_operators=["+", "-", "*", "/", "^"],
                      unary_operators=["sin", "cos", "exp", "safe_log", "safe_sqrt", "square", "cube", "abs", "neg"])
    trees = srhip.random_population(100, o, 4, T, seed=191, maxsize=15)
    X = (np.random.default_rng(192).random((4, 300)) * 2 + 0.25).astype(T)
    return o, trees, X, [row_reference(t, o, X, T) for t in trees]


@pytest.mark.parametrize("dirs", [[2], [4, 1, 3]], ids=str)
def test_routine_rules(gpu_ctx, dirs):
    """Every reverse rule that calls a routine or saves an operand, and ^ in both operands. Two trees of
    the population are singular in Float32 along the features they read: tree 22 is sqrt(x1 - |x1|) = sqrt(0),
    and tree 51's sqrt(square(log(sin(..)))) meets sin = 1 exactly on a row; both give 0·∞ in either mode."""
    o, trees, X, refs = routine_population()
    ok = check_against_both(gpu_ctx, trees, o, X, refs, dirs, L2, 0.0, 193, 100, f"routines {dirs}", singular=3)
    assert ok.sum() >= 40


def test_mixed_batch(gpu_ctx):
    """tanh has no reverse rule: its tree runs in the interpreter kernel of the same call."""
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "tanh"])
    B, U, x = o.make_binary, o.make_unary, lambda k: Node(f"x{k}")
    trees = [B("*", x(1), x(2)), U("tanh", B("*", x(1), x(2))), B("+", U("cos", x(1)), B("*", x(2), x(2))),
             B("/", U("exp", x(3)), B("+", x(1), Node(val=2.5)))]
    X = (np.random.default_rng(194).random((4, 300)) + 0.5).astype(T)
    refs = [row_reference(t, o, X, T) for t in trees]
    ok = check_against_both(gpu_ctx, trees, o, X, refs, [2, 1], L2, 0.0, 195, len(trees) - 1, "mixed")
    assert ok.all()


def test_flag_rule_and_padding(gpu_ctx):
    """sqrt(x1*x1) at x1 = 0: the value is finite, the derivative is not, so ok = 1 with a non-finite
    channel 1 (the interpreter's rule). Without the zero row the sum is finite: rows past 300 are masked."""
    o = srhip.Options(binary_operators=["+", "*"], unary_operators=["safe_sqrt"])
    tree = o.make_unary("safe_sqrt", o.make_binary("*", Node("x1"), Node("x1")))
    X = np.linspace(0.5, 2.0, 600).astype(T).reshape(2, 300)
    Y = np.ones((2, 300), dtype=T)
    sums, ok, ncode, _ = run(gpu_ctx, [tree], o, X, Y, None, [1])
    assert ncode == 1 and ok[0] and np.isfinite(sums[0]).all()
    X[0, 0] = 0.0
    sums, ok, ncode, _ = run(gpu_ctx, [tree], o, X, Y, None, [1])
    assert ncode == 1 and ok[0] and np.isfinite(sums[0, 0]) and not np.isfinite(sums[0, 1])


def test_varying_constants(gpu_ctx):
    """The code reads its constants from memory: set_constants is followed with nothing rebuilt."""
    o, trees, X, _ = population(T)
    trees = trees[:40]
    dirs = [3, 1]
    Y, W = make_targets(X, dirs, T, 196)
    flat = srhip.flatten(trees, o, dtype=T)
    ds = MultiDeviceDataset(gpu_ctx, X, Y, W)
    prog = Program(gpu_ctx, flat, T, varying_constants=True, interpreted=True, deriv_tree_code=True)
    first, _, _ = prog.eval_loss_deriv(ds, L2, [d - 1 for d in dirs])
    new = (np.asarray(flat.consts, dtype=T) * T(1.25) + T(0.125)).astype(T)
    prog.set_constants(new)
    sums, _, ok = prog.eval_loss_deriv(ds, L2, [d - 1 for d in dirs])
    assert gpu_ctx.last_tree_code() == 40 and prog.update_stats()["rebuilt"] == 0
    plain = Program(gpu_ctx, flat, T, varying_constants=True, interpreted=True)
    plain.set_constants(new)
    _, _, rok = plain.eval_loss_deriv(ds, L2, [d - 1 for d in dirs])
    assert np.array_equal(ok, rok) and ok.sum() >= 20 and not np.array_equal(first, sums, equal_nan=True)
    refs = []
    for t, tr in enumerate(trees):  # the oracle on the trees with the new constants
        tr = tr.copy()
        srhip.set_constants(tr, new[flat.const_off[t]:flat.const_off[t + 1]])
        refs.append(row_reference(tr, o, X, T))
    assert check_channels(sums, ok, refs, dirs, Y, W, T, msg="new constants") == int(ok.sum()) * 2


def test_five_directions_stay_interpreted(gpu_ctx):
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    trees = srhip.random_population(40, o, 6, T, seed=94)
    X = np.random.default_rng(95).standard_normal((6, 300)).astype(T)
    dirs = [2, 5, 1, 6, 3]
    Y, W = make_targets(X, dirs, T, 96)
    sums, ok, ncode, name = run(gpu_ctx, trees, o, X, Y, W, dirs)
    ref, rok, _, _ = run(gpu_ctx, trees, o, X, Y, W, dirs, tree_code=False)
    assert (ncode, name) == (0, "grad_kernel_deriv<float>")
    assert np.array_equal(ok, rok) and np.array_equal(sums, ref, equal_nan=True)
