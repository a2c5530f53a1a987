"""The FAST region's packed divisions check a lower bound only (csrc/gen_jit.py
manual_div_fast, manual_div_lc_fast, manual_div_rk_fast: min(|numerator|,
|rcp(divisor)|) >= 2^-50), and a FAST-eligible tree whose only routine calls
are divisions now starts in the FAST region (csrc/jit.cpp Gen::analyze).

  * values: every quotient a kept tile returns is numpy's Float32 quotient bit
    for bit, over the whole normal exponent range, on the bound itself, with a
    zero or a denormal numerator in the tile and at the mantissa edges, for
    x0 / x1, c / x0 and x0 / c, in division-only trees and in trees that hold
    an exp, with the FAST path on and off;
  * verdicts: a row whose packed quotient overflows, or whose divisor is zero,
    denormal, infinite or NaN, gives the did_succeed of the oracle and of the
    compiled routines (SRHIP_JIT_MANUAL=0), also where a later operation would
    absorb the non-finite value (exp(-q), x2 / q, q * 0);
  * a random population on mixed magnitudes equals the compiled routines.

Tiles are 256 rows (one wave, four rows per lane); inputs are built tile by
tile, so that a tile sent to the compiled routine cannot hide the packed path
of another.
"""
import os

import numpy as np
import pytest

import oracle
import srhip
from srhip import constants as K

pytestmark = pytest.mark.gpu

T = 256          # rows of a tile
LOG2_BOUND = -50  # gen_jit.py DIV_FAST_MIN
F32 = np.float32
CFG2 = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(trees, o, X, y, fast="1", **kv):
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    flat = srhip.flatten(trees, o, dtype=np.float32)
    with env(SRHIP_JIT="1", SRHIP_JIT_FAST=fast, **kv):
        prog = srhip.Program(ctx, flat, np.float32)
        sums, wsum, ok = prog.eval_loss(ds, K.LOSS["L2"])
        info = prog.jit_info()
        redone = ctx.last_jit_events()[1]
    return np.array(sums, copy=True), np.array(ok, copy=True), info, redone


# ---- value tests ----------------------------------------------------------------

def _mag(rng, lo, hi, n=T):
    """Random signs and significands, exponents uniform in lo .. hi."""
    v = rng.uniform(1, 2, n) * np.exp2(rng.integers(lo, hi + 1, n).astype(np.float64))
    return (v * rng.choice([-1, 1], n)).astype(F32)


def _tiles(rng, nrange, keep):
    """(a, b) tiles: nrange over the whole normal exponent range (those `keep`
    admits), interleaved with the bound, zero, denormal and mantissa-edge
    tiles. keep(a, b) says whether a whole-range tile suits the tree family."""
    lo = F32(2.0 ** LOG2_BOUND)
    hi = F32(2.0 ** -LOG2_BOUND)
    edges = np.array([float.fromhex("0x1.fffffep0"), float.fromhex("0x1.000002p0"), 1.0])
    out = []
    k = 0
    while sum(1 for t in out if t[2] == "range") < nrange:
        # one exponent pair per tile (a row-wise draw would leave no tile whose quotients are
        # all normal), each row within a binade of it, over the whole normal range
        ea, eb = rng.integers(-126, 128, 2)
        a = _mag(rng, max(ea - 1, -126), min(ea + 1, 127))
        b = _mag(rng, max(eb - 1, -126), min(eb + 1, 127))
        if not keep(a, b):
            continue
        out.append((a, b, "range"))
        kind = k % 7
        k += 1
        # on the bound: |a| in [2^-50, 2^-49), |b| in [2^49, 2^50], some rows exactly on it
        a = _mag(rng, LOG2_BOUND, LOG2_BOUND)
        b = _mag(rng, -LOG2_BOUND - 1, -LOG2_BOUND - 1)
        r = rng.permutation(T)
        a[r[:8]] = lo * rng.choice([-1, 1], 8).astype(F32)
        b[r[8:16]] = hi * rng.choice([-1, 1], 8).astype(F32)
        if kind == 0:
            out.append((a, b, "on the bound"))
        elif kind == 1:    # one ulp below it: the tile goes to the compiled routine
            a[r[20]] = np.nextafter(lo, F32(0))
            out.append((a, b, "a below the bound"))
        elif kind == 2:    # |b| one ulp above 2^50: |rcp(b)| below the bound
            b[r[20]] = -np.nextafter(hi, F32(np.inf))
            out.append((a, b, "b above the bound"))
        else:
            a, b = _mag(rng, -20, 20), _mag(rng, -20, 20)
            if kind == 3:
                a[r[0]] = 0
            elif kind == 4:
                a[r[0]] = F32(2.0 ** -140) * F32(1.25)
            elif kind == 5:
                a = (rng.choice(edges, T) * np.exp2(rng.integers(-40, 41, T).astype(np.float64))).astype(F32)
                b = (rng.choice(edges, T) * np.exp2(rng.integers(-40, 41, T).astype(np.float64))
                     * rng.choice([-1, 1], T)).astype(F32)
            out.append((a, b, ["a = 0", "denormal a", "mantissa edges", "in range"][kind - 3]))
    return out


def _shapes(o, quotient, ref_feature, small_feature):
    """(quotient - reference) and the same times exp(small): division-only, and with a transcendental."""
    d = lambda: o.make_binary("-", quotient(), srhip.Node(feature=ref_feature))
    return [d(), o.make_binary("*", d(), o.make_unary("exp", srhip.Node(feature=small_feature)))]


def _check_zero_loss(trees, o, X, fast):
    y = np.zeros(X.shape[1], F32)
    s, ok, info, redone = run(trees, o, X, y, fast=fast)
    print(f"fast={fast}: {info['ntrees']} trees, {info['nfast']} FAST, {redone} tiles redone, "
          f"{int((s != 0).sum())} nonzero sums, {int((~ok).sum())} failed")
    assert info["ntrees"] == len(trees)
    # division-only trees are FAST too (they call a packed division)
    assert info["nfast"] == (len(trees) if fast == "1" else 0)
    assert ok.all(), np.flatnonzero(~ok)
    assert np.all(s == 0), (np.flatnonzero(s != 0), s[s != 0])


@pytest.fixture(scope="module")
def value_data():
    return _value_data()


# No subtree without a constant repeats six times and no exp(x_f) four times in a batch below: the
# tree compiler would move it to a shared column, computed once by PRECISE code (csrc/jit.cpp
# plan_shared, plan_columns), and the trees would hold no division or no exp any more. So x0 / x1
# stands in two trees only, and every tree with an exp has a feature of its own for it.
def _value_data():
    """Per tree family (x0 / x1, c / x0, x0 / c): the feature matrix and the constants.
    Features: the operand(s), then one reference quotient per tree pair, then one small
    column (the exp's argument) per tree pair."""
    rng = np.random.default_rng(2051)
    normal = lambda q: bool(np.all(np.isfinite(q) & (np.abs(q) >= F32(2.0 ** -126))))
    smalls = lambda k, n: rng.uniform(-1, 1, (k, n)).astype(F32)
    with np.errstate(all="ignore"):
        # x0 / x1: features a, b, a / b, small
        tl = _tiles(rng, 150, lambda a, b: normal(a / b))
        a = np.concatenate([t[0] for t in tl])
        b = np.concatenate([t[1] for t in tl])
        Xv = np.concatenate([np.stack([a, b, a / b]), smalls(1, a.size)]).astype(F32)
        # c / x0: the tiles' b is the divisor (2^-50 and 2^-46: the host sends them to the compiled routine)
        c_lc = F32([3.0, -0.1, 7.5e12, 2.0 ** 45, 2.0 ** -45, 2.0 ** -50, float.fromhex("0x1.fffffep44"), 2.0 ** -46])
        tl = _tiles(rng, 150, lambda a, b: bool(np.isfinite(c_lc[:, None] / b[None, :]).all()))
        b = np.concatenate([t[1] for t in tl])
        Xlc = np.concatenate([b[None, :], c_lc[:, None] / b[None, :], smalls(len(c_lc), b.size)]).astype(F32)
        # x0 / c: the tiles' a is the numerator (1.5 * 2^-61: outside the reciprocal routine's range)
        c_rk = F32([3.0, -0.1, 7.0, 2.0 ** 60, 2.0 ** -60, float.fromhex("0x1.fffffep0"), 1.5 * 2.0 ** -61])
        tl = _tiles(rng, 150, lambda a, b: bool(np.isfinite(a[None, :] / c_rk[:, None]).all()))
        a = np.concatenate([t[0] for t in tl])
        Xrk = np.concatenate([a[None, :], a[None, :] / c_rk[:, None], smalls(len(c_rk), a.size)]).astype(F32)
    for X in (Xv, Xlc, Xrk):
        assert np.isfinite(X).all() and X.shape[1] % T == 0 and X.shape[1] >= 290 * T
    return Xv, (Xlc, c_lc), (Xrk, c_rk)


@pytest.mark.parametrize("fast", ["1", "0"])
def test_variable_division_values(gpu_ctx, value_data, fast):
    X = value_data[0]
    o = srhip.Options(**CFG2)
    q = lambda: o.make_binary("/", srhip.Node(feature=1), srhip.Node(feature=2))
    _check_zero_loss(_shapes(o, q, 3, 4), o, X, fast)


@pytest.mark.parametrize("fast", ["1", "0"])
def test_constant_numerator_values(gpu_ctx, value_data, fast):
    X, c = value_data[1]
    o = srhip.Options(**CFG2)
    trees = []
    for j, cj in enumerate(c):
        q = lambda: o.make_binary("/", srhip.Node(val=cj), srhip.Node(feature=1))
        trees += _shapes(o, q, 2 + j, 2 + len(c) + j)
    _check_zero_loss(trees, o, X, fast)


@pytest.mark.parametrize("fast", ["1", "0"])
def test_constant_divisor_values(gpu_ctx, value_data, fast):
    X, c = value_data[2]
    o = srhip.Options(**CFG2)
    trees = []
    for j, cj in enumerate(c):
        q = lambda: o.make_binary("/", srhip.Node(feature=1), srhip.Node(val=cj))
        trees += _shapes(o, q, 2 + j, 2 + len(c) + j)
    _check_zero_loss(trees, o, X, fast)


# ---- verdict tests --------------------------------------------------------------

FMAX = float(np.finfo(np.float32).max)
# The engine takes finite features only, so an infinite or NaN operand is an intermediate result:
#   sq     x * x              +Inf in the special row (x = 2^100)
#   negsq  -(x * x)           -Inf
#   nan    (x*x - x*x) + x    NaN (Inf - Inf); x in the other rows
# The oracle fails such a tree at the operand; the tree code checks the root and marks the operands
# of the operations that can lose a non-finite value, so it has to fail it at the division
# (a / Inf = 0: b_div_full marks b) or carry the value to the root.
# (name, form of a, form of b, x0 and x1 of the one special row of the kind's second tile)
KINDS = [
    ("b = +0", "raw", "raw", 1.5, 0.0), ("b = -0", "raw", "raw", 1.5, -0.0),
    ("b = +Inf", "raw", "sq", 1.5, 2.0 ** 100), ("b = -Inf", "raw", "negsq", -1.5, 2.0 ** 100),
    ("denormal b, finite quotient", "raw", "raw", 1.25 * 2.0 ** -10, 2.0 ** -130),
    ("a = +Inf", "sq", "raw", 2.0 ** 100, 1.5), ("a = -Inf", "negsq", "raw", 2.0 ** 100, 1.5),
    ("NaN a", "nan", "raw", 2.0 ** 100, 1.5), ("NaN b", "raw", "nan", 1.5, 2.0 ** 100),
    ("quotient overflows", "raw", "raw", 2.0 ** 100, -(2.0 ** -100)),
    ("quotient an ulp below the largest", "raw", "raw", FMAX, float.fromhex("0x1.000002p0")),
]
NROWS = 4 * T
SPECIAL = T + 37


def _form_value(form, x):
    with np.errstate(all="ignore"):
        return {"raw": lambda: x, "sq": lambda: x * x, "negsq": lambda: -(x * x),
                "nan": lambda: ((x * x) - (x * x)) + x}[form]()


def _form_tree(o, form, f):
    N = srhip.Node
    sq = lambda: o.make_binary("*", N(feature=f), N(feature=f))
    if form == "raw":
        return N(feature=f)
    if form == "sq":
        return sq()
    if form == "negsq":
        return o.make_unary("neg", sq())
    return o.make_binary("+", o.make_binary("-", sq(), sq()), N(feature=f))


def _verdict_problem():
    rng = np.random.default_rng(2052)
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp", "neg"])
    N = srhip.Node
    cols, trees, names = [], [], []
    for k, (name, fa, fb_, sa, sb) in enumerate(KINDS):
        x0 = rng.uniform(0.5, 2.0, NROWS) * rng.choice([-1, 1], NROWS)
        x1 = rng.uniform(0.5, 2.0, NROWS) * rng.choice([-1, 1], NROWS)
        x0[SPECIAL], x1[SPECIAL] = sa, sb
        x0, x1 = x0.astype(F32), x1.astype(F32)
        with np.errstate(all="ignore"):
            q = _form_value(fa, x0) / _form_value(fb_, x1)
        x2 = np.where(np.isfinite(q) & (q != 0), q, F32(1)).astype(F32)
        f = 1 + 3 * k  # features x0, x1, x2 of this kind
        cols += [x0, x1, x2]
        A = lambda: _form_tree(o, fa, f)
        B = lambda: _form_tree(o, fb_, f + 1)
        X2 = lambda: N(feature=f + 2)
        zero, three = lambda: N(val=F32(0)), lambda: N(val=F32(3))
        q_ = lambda: o.make_binary("/", A(), B())
        ts = [
            ("exp(-(a/b))", o.make_unary("exp", o.make_unary("neg", q_()))),
            ("x2/(a/b)", o.make_binary("/", X2(), q_())),
            ("(a/b)*0", o.make_binary("*", q_(), zero())),
            ("(a/b)-x2", o.make_binary("-", q_(), X2())),
            ("(3/b)*0", o.make_binary("*", o.make_binary("/", three(), B()), zero())),
            ("x2/(3/b)", o.make_binary("/", X2(), o.make_binary("/", three(), B()))),
            ("exp(-(a/3))", o.make_unary("exp", o.make_unary("neg", o.make_binary("/", A(), three())))),
            ("(a/3)*0", o.make_binary("*", o.make_binary("/", A(), three()), zero())),
        ]
        for tn, t in ts:
            trees.append(t)
            names.append(f"{name}: {tn}")
    X = np.stack(cols).astype(F32)
    assert np.isfinite(X).all()
    y = np.zeros(NROWS, F32)
    return o, trees, names, X, y


@pytest.fixture(scope="module")
def verdict_problem():
    o, trees, names, X, y = _verdict_problem()
    flat = srhip.flatten(trees, o, dtype=np.float32)
    ref_sum, _, ref_ok = oracle.eval_loss_batch(flat, X, y, dtype=np.float32)
    return o, trees, names, X, y, ref_sum, ref_ok


@pytest.mark.parametrize("fast", ["1", "0"])
def test_division_verdicts(gpu_ctx, verdict_problem, fast):
    """did_succeed and the sums of every tree equal the oracle's and those of
    the compiled routines (SRHIP_JIT_MANUAL=0).

    The oracle sums l = ŷ² (Float32) in Float64; the tree code adds fma(ŷ, ŷ, sum)
    in Float32, 1024 rows per tree: at most (n + 2) * 2^-24 relative for the n
    non-negative terms, plus 2 * 2 ulp of ŷ for the trees with an exp, whose
    Float32 exp is within 2 ulp of the oracle's."""
    o, trees, names, X, y, ref_sum, ref_ok = verdict_problem
    s, ok, info, redone = run(trees, o, X, y, fast=fast)
    s0, ok0, info0, _ = run(trees, o, X, y, fast=fast, SRHIP_JIT_MANUAL="0")
    print(f"fast={fast}: {info['ntrees']} trees, {info['nfast']} FAST, {redone} tiles redone")
    for i in np.flatnonzero((ok != ref_ok) | (ok != ok0)):
        print(f"  {names[i]}: ok {ok[i]} oracle {ref_ok[i]} compiled routines {ok0[i]}")
    rtol = (NROWS + 2) * 2.0 ** -24 + 4 * 2.0 ** -23
    both = ok & ref_ok
    m = both & np.isfinite(ref_sum)  # (a finite ŷ whose square overflows: an infinite sum, ok = 1, in both)
    rel = np.abs(s[m] - ref_sum[m]) / np.maximum(np.abs(ref_sum[m]), 1e-300)
    print(f"  sums against the oracle: max relative difference {rel.max():.3g} (bound {rtol:.3g})")
    assert info["ntrees"] == info0["ntrees"] == len(trees)
    assert np.array_equal(ok, ok0), [names[i] for i in np.flatnonzero(ok != ok0)]
    assert np.array_equal(s[ok], s0[ok0])
    assert np.array_equal(ok, ref_ok), [names[i] for i in np.flatnonzero(ok != ref_ok)]
    assert np.array_equal(np.isfinite(s[both]), np.isfinite(ref_sum[both]))
    assert np.all(rel <= rtol), [names[i] for i in np.flatnonzero(m)[rel > rtol]]
    # what the rows are there for
    by = {n_: bool(k_) for n_, k_ in zip(names, ok)}
    for kd in ("b = +Inf", "b = -Inf"):  # the quotient is 0 and the tree fails
        for tn in ("exp(-(a/b))", "x2/(a/b)", "(a/b)*0", "(a/b)-x2", "(3/b)*0", "x2/(3/b)"):
            assert not by[f"{kd}: {tn}"], (kd, tn)
    for kd in ("denormal b, finite quotient", "quotient an ulp below the largest"):
        assert by[f"{kd}: (a/b)*0"] and by[f"{kd}: (a/b)-x2"]
        assert s[names.index(f"{kd}: (a/b)-x2")] == 0  # numpy's quotient, bit for bit
    for kd in ("b = +0", "b = -0", "a = +Inf", "a = -Inf", "NaN a", "NaN b", "quotient overflows"):
        for tn in ("exp(-(a/b))", "x2/(a/b)", "(a/b)*0", "(a/b)-x2"):
            assert not by[f"{kd}: {tn}"], (kd, tn)


# ---- a random population --------------------------------------------------------

def test_random_population_equals_compiled_routines(gpu_ctx):
    o = srhip.Options(binary_operators=["+", "-", "*", "/"],
                      unary_operators=["sin", "cos", "exp", "square", "cube", "neg"])
    trees = srhip.random_population(1500, o, 5, np.float32, seed=41)
    rng = np.random.default_rng(42)
    X = (rng.standard_normal((5, 60_000)) * rng.choice([1e-3, 1.0, 30.0, 1e4], (5, 60_000))).astype(np.float32)
    X[:, :256] = rng.uniform(0.5, 2.0, (5, 256)).astype(np.float32)  # one tile with every division in range
    y = (np.float32(2) * np.cos(X[3]) + X[0] * X[0] - np.float32(2)).astype(np.float32)
    for fast in ("1", "0"):
        s_m, ok_m, info_m, redone = run(trees, o, X, y, fast=fast)
        s_f, ok_f, info_f, _ = run(trees, o, X, y, fast=fast, SRHIP_JIT_MANUAL="0")
        print(f"fast={fast}: {info_m['ntrees']} trees, {info_m['nfast']} FAST ({info_f['nfast']} with the compiled "
              f"routines), {redone} tiles redone, {int(ok_m.sum())} succeeded")
        assert info_m["ntrees"] == info_f["ntrees"] > 1000
        assert np.array_equal(ok_m, ok_f)
        assert np.array_equal(s_m[ok_m], s_f[ok_f])
