"""Every operator's derivative rule in the forward-mode interpreter (device_ops.h uop_d / bop_d,
grad_interp.h un_grad / bin_grad / loss_bin_dual) against the independent fixture
tests/golden/derivatives.npz, and against the oracle in T.

These rules run in the interpreter only: the gradient tree code compiles `+ - * /` and neg abs square cube
exp sin cos log sqrt (jit_grad.cpp kGradUops) with rules of its own (pinned to the same fixture by
test_operator_values_gpu.test_gradient_tree_code_rules), and every batch here is far below its
bar, which pass_info (grad_rest) and last_tree_code assert.

All cases use 293 rows (derivative_cases.NROWS). Constants that only carry a tangent are -0.0 or 1.0, so
the operand is the grid value bit for bit.

Bounds (nothing fitted to the engine's results):
  against the oracle in T, Float64: rtol = atol = 1e-10, the per-row bar of
      test_gradients.test_many_constants_and_deep_trees;
  against the fixture: B = oracle_err_ulp + 4 ulp of T per transcendental value that enters the rule
      multiplicatively + 2 ulp for the rule's divide (counts next to each rule in make_derivative_golden.py),
      in ulps of T of the true partial, plus assert_close_conditioned's term, 4 x the movement of the true
      partial under a 4-ulp move of the operand; where a partial P is multiplied by an exact tangent m the
      bound is |m| times that plus 1 ulp of T of P·m for the multiply (tangent sums add exact zeros);
  against the oracle in T, Float32: the oracle is within oracle_err_ulp of the truth and the engine within B,
      so B + oracle_err_ulp (+ conditioning), by the triangle inequality.
  loss gradients (sums over rows; the wide, row-set, target and expression-loss slices): the per-row bounds
      summed, plus RTOL·Σ|terms| for the sum itself, which the kernels accumulate in T per lane
      (test_margin_losses_gpu.RTOL, the bar of test_variant_matrix_gpu's loss gradients: 1e-5 Float32,
      1e-9 Float64). That term dominates: this is not a per-row bound. These slices catch a wrong rule or a
      wrong tangent combination on their path (measured worst ratios are about 0.01), not an error at the
      ulp level; the ulp-level checks are the per-row matrices above.
Every point is checked (max_bad_frac = 0), and every grid point's bound is finite but for two Float32 acosh
operands next to 1 (test_derivative_rules.test_every_grid_point_has_a_finite_bound). The worst error / bound
per (operator, dtype, path) goes to numerics.record_tail (profiles/derivative_rules_parity.json holds a
run's figures).
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import derivative_cases as D
import numerics
import oracle
import srhip
from srhip import Node
from test_margin_losses_gpu import RTOL

pytestmark = pytest.mark.gpu

NROWS = D.NROWS
TIDS = dict(ids=lambda T: np.dtype(T).name)
GX, GY, GW = 1, 2, 3  # features of a binary case: grid x, grid y, a positive multiplier
NONCOMM = ("-", "/", "pow", "mod", "max", "min")


@contextlib.contextmanager
def env(**kw):
    """Set for a block and restored (the engine reads its switches per call), as test_variant_matrix_gpu.env."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        os.environ.update(kw)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def B(op, l, r):
    return D.options().make_binary(op, l, r)


def feat(f):
    return Node(feature=f)


def scaled(f, c=1.0):
    """x_f * c: a computed operand whose value is x_f (c = 1.0) and whose tangent is x_f."""
    return B("*", feat(f), Node(val=c))


# ---- comparison ------------------------------------------------------------------------

def as_T_class(d, T):
    """The true value with T's overflow applied (an Inf where T rounds it to one)."""
    with np.errstate(over="ignore"):
        dT = np.asarray(d, dtype=np.float64).astype(T).astype(np.float64)
    return np.where(np.isinf(dT), dT, d)


def check(got, ref, tol, what):
    """Every element: |got - ref| <= tol, equal infinities and NaN pairs agree. Returns the worst err / tol."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    numerics.assert_close_conditioned(got, ref, tol, rtol=0.0, atol=0.0, factor=1.0, msg=what, max_bad_frac=0.0)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        ratio = np.where((got == ref) | (np.isnan(got) & np.isnan(ref)), 0.0, err / tol)
    return float(np.nanmax(ratio)) if ratio.size else 0.0


def partial_tol(P, spread, bulp, T, m=1.0):
    """|m| (bulp ulp_T(P) + 4 spread) + 1 ulp_T(P m) when a tangent multiplies (module docstring)."""
    m = np.abs(np.asarray(m, dtype=np.float64))
    with np.errstate(invalid="ignore"):  # a zero tangent times an infinite spread: the term is exactly 0
        tol = np.where(m == 0, 0.0, m * (bulp * D.ulp_of(P, T) + 4.0 * spread))
    if np.ndim(m) or m != 1.0:
        tol = tol + D.ulp_of(P * m, T)
    return tol


def oracle_spread(op, x, T):
    """The movement of the oracle's Float64 derivative under a 4-ulp-of-T move of the operand (for the rows
    the fixture does not hold: in-domain fill, away from poles)."""
    eps4 = 4 * float(np.finfo(T).eps)
    _, d0, ok = D.oracle_unary_d(op, x, np.float64)
    assert ok
    sp = np.zeros_like(d0)
    for s in (1 + eps4, 1 - eps4):
        _, d1, ok = D.oracle_unary_d(op, x * s, np.float64)
        assert ok
        sp = np.maximum(sp, np.abs(d1 - d0))
    return sp


class Tails:
    def __init__(self, path, T):
        self.path, self.T, self.worst = path, np.dtype(T).name, {}

    def add(self, op, ratio):
        self.worst[op] = max(self.worst.get(op, 0.0), float(ratio))

    def flush(self):
        assert all(v <= 1.0 for v in self.worst.values()), self.worst
        numerics.record_tail("derivative_rules", dict(path=self.path, dtype=self.T, worst_err_over_bound=self.worst))
        print(f"{self.path} {self.T}: worst err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.items())))


# ---- a. the unary matrix ---------------------------------------------------------------

def unary_batch(which):
    basic = [o for o in D.unary_ops() if o in D.BASIC_UNARY]
    others = [o for o in D.unary_ops() if o not in D.BASIC_UNARY] + D.zero_unary()
    return {"shallow-basic": basic, "shallow-full": others, "deep": basic + others}[which]


def unary_problem(ops, T, deep, seed=600):
    """One tree op(c0 + x_i) per operator, each on its own feature; the last feature feeds the deep pad."""
    nf = len(ops) + 1
    X = np.empty((nf, NROWS))
    grids = {}
    for i, op in enumerate(ops):
        if op in D.zero_unary():
            g = np.array(sorted({x for o, x, _ in D.conv_unary(T) if o == op}))
        else:
            g = D.unary_case(op, T)[0]
        grids[op] = g
        X[i] = D.rows_with_fill(g, op, T, seed + i)
    X[nf - 1] = np.random.default_rng(seed - 1).uniform(0.5, 1.5, NROWS)
    trees = []
    for i, op in enumerate(ops):
        t = D.unary_tree(op, i + 1)
        # deep: the same node inside a tree that needs 5 stack slots. The pad is feature-only and added
        # with `+` (both partials 1, its tangent 0): ∂ŷ/∂c0 is still op'(x) exactly.
        trees.append(B("+", t, D.pad_tree(nf)) if deep else t)
    return trees, X.astype(T), grids


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
@pytest.mark.parametrize("which", ["shallow-basic", "shallow-full", "deep"])
def test_unary_matrix(gpu_ctx, which, T):
    """op(c0 + x) for every unary operator through eval_grad_tree_array: ∂ŷ/∂c0 per row against the fixture
    (grid rows) and the oracle in T (every row), in the shallow BASIC, shallow FULL and deep kernels."""
    ctx = gpu_ctx
    ops = unary_batch(which)
    deep = which == "deep"
    trees, X, grids = unary_problem(ops, T, deep)
    flat = srhip.flatten(trees, D.options(), dtype=T)
    assert list(np.diff(flat.const_off)) == [1] * len(ops)
    prog = srhip.Program(ctx, flat, T)
    val, grad, ok = prog.eval_grad_tree_array(srhip.DeviceDataset(ctx, X, np.zeros(NROWS, dtype=T)))
    assert ctx.last_tree_code() == 0
    info = prog.pass_info()
    assert info["grad_rest"] == (0, 0, 0, 0), info
    if deep:  # the deep item count: one item per tree, none in the shallow passes
        assert info["grad_items"] == (0, 0, 0, len(ops)), info
    else:
        assert info["grad_items"] == (len(ops), 0, 0, 0), info
        assert info["grad_opset"] == ("BASIC" if which == "shallow-basic" else "FULL"), info
    assert ok.all(), [op for op, k in zip(ops, ok) if not k]
    fx_t, or_t = Tails(f"unary {which} vs fixture", T), Tails(f"unary {which} vs oracle", T)
    for i, op in enumerate(ops):
        x = X[i].astype(np.float64)
        v, g_or, okr = D.oracle_unary_d(op, x, T)
        assert okr, op
        got = grad[i].astype(np.float64)
        if op in D.zero_unary():
            assert not got.any() and not g_or.any(), (op, got[got != 0])
            continue
        n = len(grids[op])
        _, d, spread = D.unary_case(op, T)
        assert np.array_equal(x[:n], grids[op])
        bulp = D.unary_bound_ulp(op, T)
        what = f"{op} {np.dtype(T).name} {which}"
        fx_t.add(op, check(got[:n], as_T_class(d, T), partial_tol(d, spread, bulp, T), what + " vs fixture"))
        if T == np.float64:
            np.testing.assert_allclose(got, g_or, rtol=1e-10, atol=1e-10, err_msg=what)
            or_t.add(op, np.nanmax(np.where(got == g_or, 0.0, np.abs(got - g_or) / (1e-10 + 1e-10 * np.abs(g_or)))))
        else:
            sp = np.concatenate([spread, oracle_spread(op, x[n:], T)])
            oerr = float(D.fixture()[f"una/{op}/f32/oracle_err_ulp"])
            or_t.add(op, check(got, g_or, partial_tol(g_or, sp, bulp + oerr, T), what + " vs oracle"))
    fx_t.flush()
    or_t.flush()


# ---- b. the binary matrix --------------------------------------------------------------
# Each shape is the one compile.cpp's TreeCompiler::emit turns into that bin_grad variant.

def shape(variant, op, const=None):
    """(tree, terms): terms[k] = (partial "x" / "y" / None, multiplier feature or None) of constant k in
    get_constants (preorder) order: ∂ŷ/∂c_k = partial · multiplier; (None, GW) is the sibling constant."""
    c = (lambda v: Node(val=v))
    if variant == "V_XC":  # two leaves, feature then constant: emit's `else if (L.feat >= 0) putc(V_XC ...)`
        return B(op, feat(GX), c(const)), [("y", None)]
    if variant == "V_CX":  # two leaves, constant then feature: `else if (R.feat >= 0) putc(V_CX ...)`
        return B(op, c(const), feat(GY)), [("x", None)]
    if variant == "V_AX":  # computed left, feature right: `if (is_leaf(R)) { emit(x.l); if (R.feat >= 0) put(V_AX ...`
        return B(op, scaled(GX), feat(GY)), [("x", GX)]
    if variant == "V_XA":  # feature left, computed right: `if (is_leaf(L)) { emit(x.r); if (L.feat >= 0) put(V_XA ...`
        return B(op, feat(GX), scaled(GY)), [("y", GY)]
    if variant == "V_AC":  # computed left, constant right: `if (is_leaf(R)) ... else putc(V_AC, R)`
        return B(op, scaled(GX), c(const)), [("x", GX), ("y", None)]
    if variant == "V_CA":  # constant left, computed right: `if (is_leaf(L)) ... else putc(V_CA, L)`
        return B(op, c(const), scaled(GY)), [("x", None), ("y", GY)]
    if variant == "V_AT":
        # two computed operands, the right one needing more stack (need 1 against 0): `lf = L.need >= R.need`
        # is false, the right side is emitted first and pushed: `put(V_AT ...)  // lhs = acc (left), rhs = tmp`.
        # x_GY·1.0 + x_GW·(-0.0) == x_GY bit for bit (x_GW > 0).
        return (B(op, scaled(GX), B("+", scaled(GY), scaled(GW, -0.0))),
                [("x", GX), ("y", GY), ("y", GW)])
    if variant == "V_TA":  # the heavier side on the left: emitted first, `put(V_TA ...)  // lhs = tmp (left), rhs = acc`
        return (B(op, B("+", scaled(GX), scaled(GW, -0.0)), scaled(GY)),
                [("x", GX), ("x", GW), ("y", GY)])
    assert variant == "V_XX"
    # two feature leaves: `put_feat2(V_XX ...)`, here as the right operand of a sum whose left operand
    # (c0 · x_GW, tangent x_GW) is still in the accumulator when V_XX runs: V_XX has to start from zero
    # tangents. If it kept the accumulator's, ∂ŷ/∂c0 would come out as 2 x_GW.
    return B("+", B("*", Node(val=1.0), feat(GW)), B(op, feat(GX), feat(GY))), [(None, GW)]


VARIANTS = ["V_XC", "V_CX", "V_AX", "V_XA", "V_AC", "V_CA", "V_AT", "V_TA", "V_XX"]
GRAD_PASS = {1: 0, 2: 1, 3: 2}  # constants of the tree -> the G = 1, 2, 4 pass (one work item)


def binary_blocks(op, T):
    """Per block of the operator's grid: (X [3][NROWS] as float64, index of each row's pair in the fixture
    arrays). The rows repeat the block's pairs, so every row is a grid point."""
    c = D.binary_case(op, T)
    rng = np.random.default_rng(77)
    for b in np.unique(c["block"]):
        idx = np.flatnonzero(c["block"] == b)
        rows = idx[np.arange(NROWS) % len(idx)]
        w = rng.uniform(0.5, 2.0, NROWS).astype(np.float32).astype(np.float64)
        yield np.stack([c["x"][rows], c["y"][rows], w]), rows, c


def pair_index(c):
    return {(float(x), float(y)): i for i, (x, y) in enumerate(zip(c["x"], c["y"]))}


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("op", D.binary_ops())
def test_binary_matrix(gpu_ctx, op, variant, T):
    """Every binary operator through every bin_grad variant: the chain rule from the fixture's partials in
    Float64, and the oracle in T. For the piecewise-constant operators the gradient through the operator
    is exactly 0; the gradient of a sibling constant (V_XX's shape) is exact for every operator."""
    ctx = gpu_ctx
    bx, by = D.binary_bound_ulp(op, T)
    fx_t, or_t = Tails(f"binary {variant} vs fixture", T), Tails(f"binary {variant} vs oracle", T)
    for X, rows, c in binary_blocks(op, T):
        look = pair_index(c)
        if variant in ("V_XC", "V_AC"):
            consts = sorted(set(X[1]))
        elif variant in ("V_CX", "V_CA"):
            consts = sorted(set(X[0]))
        else:
            consts = [None]
        built = [shape(variant, op, k) for k in consts]
        trees, terms = [t for t, _ in built], built[0][1]
        flat = srhip.flatten(trees, D.options(), dtype=T)
        nc = len(terms)
        assert list(np.diff(flat.const_off)) == [nc] * len(trees)
        prog = srhip.Program(ctx, flat, T)
        XT = X.astype(T)
        val, grad, ok = prog.eval_grad_tree_array(srhip.DeviceDataset(ctx, XT, np.zeros(NROWS, dtype=T)))
        assert ctx.last_tree_code() == 0 and ok.all(), (op, variant, ok)
        info = prog.pass_info()
        items = [0, 0, 0, 0]
        items[GRAD_PASS[nc]] = len(trees)
        assert info["grad_items"] == tuple(items) and info["grad_rest"] == (0, 0, 0, 0), info
        assert info["grad_opset"] == ("BASIC" if op in D.BASIC_BINARY else "FULL"), info
        for t, k in enumerate(consts):
            # the fixture point of every row: a constant operand replaces that coordinate
            px = X[0] if variant not in ("V_CX", "V_CA") else np.full(NROWS, k)
            py = X[1] if variant not in ("V_XC", "V_AC") else np.full(NROWS, k)
            at = np.array([look[(float(a), float(b))] for a, b in zip(px, py)])
            _, g_or, okr = D.oracle_grad(trees[t], XT, T)
            assert okr
            for j, (which, mf) in enumerate(terms):
                got = grad[t * nc + j].astype(np.float64)
                what = f"{op} {variant} {np.dtype(T).name} const {j} ({which}, x{mf}) tree {t}"
                m = 1.0 if mf is None else X[mf - 1]
                if which is None:  # the sibling constant: exactly x_GW, in the engine and in the oracle
                    assert np.array_equal(got, X[GW - 1]) and np.array_equal(g_or[j], X[GW - 1]), what
                    continue
                P, sp, bulp = (c["dx"][at], c["sx"][at], bx) if which == "x" else (c["dy"][at], c["sy"][at], by)
                if op in D.zero_binary():
                    assert not got.any() and not g_or[j].any(), what
                    continue
                fx_t.add(op, check(got, as_T_class(P * m, T), partial_tol(P, sp, bulp, T, m), what + " vs fixture"))
                if T == np.float64:
                    np.testing.assert_allclose(got, g_or[j], rtol=1e-10, atol=1e-10, err_msg=what)
                    with np.errstate(all="ignore"):
                        or_t.add(op, np.nanmax(np.where(got == g_or[j], 0.0,
                                                        np.abs(got - g_or[j]) / (1e-10 + 1e-10 * np.abs(g_or[j])))))
                else:
                    oerr = float(D.fixture()[f"bin/{op}/f32/oracle_err_ulp"][0 if which == "x" else 1])
                    or_t.add(op, check(got, g_or[j], partial_tol(P, sp, bulp + oerr + 1.0, T, m), what + " vs oracle"))
    fx_t.flush()
    or_t.flush()


# ---- c. the other tangent paths --------------------------------------------------------

def slice_problem(T):
    """The non-basic unary batch (op(c0 + x_i)) and the non-commutative binaries (op(x·c0, y), V_AX) on
    grid points whose value and derivative stay below 1e6 in magnitude (an L2 sum of squares must stay
    finite in Float32; this slice is about the tangent path, the unary matrix holds the extremes).
    Returns trees, X, and per tree the true ∂ŷ/∂c0 per row with its bound (both float64)."""
    ops = [o for o in D.unary_ops() if o not in D.BASIC_UNARY] + D.zero_unary()
    nf = len(ops) + 2 * len(NONCOMM)
    X = np.empty((nf, NROWS))
    trees, true, tol = [], [], []
    for i, op in enumerate(ops):
        if op in D.zero_unary():
            x = np.array(sorted({x for o, x, _ in D.conv_unary(T) if o == op}))
            d = sp = np.zeros_like(x)
            bulp = 0.0
        else:
            x, d, sp = D.unary_case(op, T)
            with np.errstate(all="ignore"):
                v = oracle.eval_tree(*srhip.flatten([D.unary_tree(op)], D.options(), dtype=np.float64).tree(0),
                                     x[None, :], dtype=np.float64)[0]
            keep = (np.abs(v) < 1e6) & (np.abs(d) < 1e6) & np.isfinite(sp)
            x, d, sp, bulp = x[keep], d[keep], sp[keep], D.unary_bound_ulp(op, T)
        r = np.arange(NROWS) % len(x)
        X[i] = x[r]
        trees.append(D.unary_tree(op, i + 1))
        true.append(d[r])
        tol.append(partial_tol(d[r], sp[r], bulp, T))
    for k, op in enumerate(NONCOMM):
        c = D.binary_case(op, T)
        keep = np.flatnonzero((c["block"] == 0) & (np.abs(c["x"]) < 1e3) & (np.abs(c["y"]) < 1e3) & (np.abs(c["dx"]) < 1e6))
        r = keep[np.arange(NROWS) % len(keep)]
        fa, fb = len(ops) + 2 * k, len(ops) + 2 * k + 1
        X[fa], X[fb] = c["x"][r], c["y"][r]
        trees.append(B(op, scaled(fa + 1), feat(fb + 1)))
        true.append(c["dx"][r] * X[fa])
        tol.append(partial_tol(c["dx"][r], c["sx"][r], D.binary_bound_ulp(op, T)[0], T, X[fa]))
    return ops + list(NONCOMM), trees, X.astype(T), np.array(true), np.array(tol)


def l2_reference(flat, XT, y, true, tol, T, rows=None):
    """Per tree (one constant each): Σ 2 r ∂ŷ/∂c in Float64 with r = ŷ - y from the oracle's ŷ in T, and
    its bound: Σ 2|r|·tol + 2|∂ŷ/∂c|·4 ulp_T(ŷ) (the engine's ŷ is within the per-operator bar of 4 ulp, and
    the subtraction is exact or rounds once: 1 more ulp of ŷ) + 2 ulp_T of each term + RTOL Σ|terms|."""
    with np.errstate(all="ignore"):
        yhat, ok = oracle.eval_trees(flat, XT, dtype=T)
    assert ok.all()
    ref, bound = np.zeros(flat.ntrees), np.zeros(flat.ntrees)
    for t in range(flat.ntrees):
        idx = np.arange(XT.shape[1]) if rows is None else rows[t]
        r = (yhat[t][idx] - y[idx]).astype(np.float64)
        d, tl = true[t][idx], tol[t][idx]
        term = 2.0 * r * d
        ref[t] = term.sum()
        bound[t] = np.sum(2.0 * np.abs(r) * tl + 2.0 * np.abs(d) * 5.0 * D.ulp_of(yhat[t][idx].astype(np.float64), T)
                          + 2.0 * D.ulp_of(term, T)) + RTOL[np.dtype(T)] * np.abs(term).sum()
    return ref, bound


def check_l2(g, ref, bound, ops, tails, what):
    for t, op in enumerate(ops):
        if bound[t] == 0.0:
            assert g[t] == 0.0 and ref[t] == 0.0, (what, op, g[t])
        else:
            tails.add(op, check(g[t:t + 1], ref[t:t + 1], bound[t:t + 1], f"{what} {op}"))


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
def test_l2_gradients_wide_rowsets_targets(gpu_ctx, T):
    """The same rules through the tangent code of the wide kernel (SRHIP_WIDE=1), the per-tree row sets
    (grad_kernel_seg) and the per-tree targets kernel: eval_loss_grad with L2 against Σ 2 r (fixture
    derivative). Row sets are also held to the bit equality with a per-sample dataset that
    test_grad_rowsets_gpu.py fixes."""
    ctx = gpu_ctx
    L2 = srhip.L2DistLoss()
    ops, trees, XT, true, tol = slice_problem(T)
    flat = srhip.flatten(trees, D.options(), dtype=T)
    assert list(np.diff(flat.const_off)) == [1] * len(trees)
    prog = srhip.Program(ctx, flat, T, interpreted=True)
    rng = np.random.default_rng(5)
    Y = np.stack([np.zeros(NROWS), rng.uniform(-1, 1, NROWS)]).astype(T)
    # plain and wide
    for wide in (False, True):
        tails = Tails("L2 wide" if wide else "L2 plain", T)
        ds = srhip.DeviceDataset(ctx, XT, Y[1])
        with env(**({"SRHIP_WIDE": "1"} if wide else {})):
            s, g, wsum, ok = prog.eval_loss_grad(ds, L2.kind, L2.params)
            name = ctx.last_kernel_name()
        assert ("wide" in name) == wide, name
        assert ok.all() and ctx.last_tree_code() == 0
        ref, bound = l2_reference(flat, XT, Y[1], true, tol, T)
        check_l2(g, ref, bound, ops, tails, name)
        tails.flush()
    info = prog.pass_info()
    assert info["grad_items"] == (len(trees), 0, 0, 0) and info["grad_opset"] == "FULL", info
    assert info["grad_rest"] == (0, 0, 0, 0), info
    # per-tree row sets
    tails = Tails("L2 row sets", T)
    rows = np.stack([rng.choice(NROWS, 270, replace=False) for _ in trees])
    ds = srhip.DeviceDataset(ctx, XT, Y[1])
    s, g, ws, ok = prog.eval_loss_grad_rowsets(ds, L2.kind, rows, L2.params)
    assert "_seg<" in ctx.last_kernel_name() and ok.all()
    ref, bound = l2_reference(flat, XT, Y[1], true, tol, T, rows)
    check_l2(g, ref, bound, ops, tails, "row sets")
    for t in (0, len(trees) // 2, len(trees) - 1):  # bit equality with tree t's sample as a dataset
        s1, g1, w1, ok1 = prog.eval_loss_grad(srhip.DeviceDataset(ctx, np.ascontiguousarray(XT[:, rows[t]]), Y[1][rows[t]]),
                                              L2.kind, L2.params)
        assert ok1[t] and g[t:t + 1].tobytes() == g1[t:t + 1].tobytes() and s[t] == s1[t], (ops[t], g[t], g1[t])
    tails.flush()
    # per-tree targets on a 2-target dataset
    tails = Tails("L2 targets", T)
    mds = srhip.engine.MultiDeviceDataset(ctx, XT, Y)
    tg = (np.arange(len(trees)) % 2).astype(np.int32)
    s, g, wsum, ok = prog.eval_loss_grad_targets(mds, L2.kind, tg, L2.params)
    assert "targets" in ctx.last_kernel_name(), ctx.last_kernel_name()
    assert ok.all()
    for k in (0, 1):
        ref, bound = l2_reference(flat, XT, Y[k], true, tol, T)
        sel = np.flatnonzero(tg == k)
        check_l2(g[sel], ref[sel], bound[sel], [ops[i] for i in sel], tails, f"target {k}")
    tails.flush()


EXPR_UNARY = ("tan", "erf", "atanh_clip")


def _p():
    return B("+", feat(1), Node(val=-0.0))  # the prediction, computed: its value with tangent 1


def _t():
    return B("+", feat(2), Node(val=-0.0))  # the target, computed: tangent 0


# form -> (the loss tree of an operator over x1 = ŷ, x2 = y; the partial dℓ/dŷ is)
FORMS = {
    "AX": (lambda op: B(op, _p(), feat(2)), "x"),       # LOP_AX: acc ∘ leaf, the tangent on the accumulator
    "XA": (lambda op: B(op, feat(2), _p()), "y"),       # LOP_XA: leaf ∘ acc
    "TA-left": (lambda op: B(op, _p(), _t()), "x"),     # LOP_TA: tmp ∘ acc, the tangent on tmp
    "TA-right": (lambda op: B(op, _t(), _p()), "y"),    # LOP_TA: the tangent on the accumulator
    # the ŷ leaf itself as an operand: loss_bin_dual's `xd ? fx` and `xd ? nd + fy` terms
    "XA-leaf": (lambda op: B(op, feat(1), _t()), "x"),  # LOP_XA: ŷ ∘ acc, the tangent on the leaf
    "AX-leaf": (lambda op: B(op, _t(), feat(1)), "y"),  # LOP_AX: acc ∘ ŷ
}


@functools.lru_cache(maxsize=None)
def expr_loss(op, form):
    """One registered handle per loss expression and process."""
    o = D.options()
    return srhip.ExprLoss(o.make_unary(op, feat(1)) if form is None else FORMS[form][0](op), o)


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
def test_expression_loss_duals(gpu_ctx, T):
    """run_loss_dual: the non-commutative binaries in each of loss_bin_dual's operand forms (acc ∘ leaf,
    leaf ∘ acc, tmp ∘ acc in both orders) and three non-basic unary operators, as a custom loss over (ŷ, y).
    The candidate tree is c0 · x1 with c0 = 1: ŷ = x1 and ∂ŷ/∂c0 = x1, so ∂L/∂c0 = Σ dℓ/dŷ · x1, checked
    against the fixture's partial at (ŷ, y) in Float64."""
    ctx = gpu_ctx
    o = D.options()
    prog = srhip.Program(ctx, srhip.flatten([B("*", Node(val=1.0), feat(1))], o, dtype=T), T)
    tails = Tails("expression loss", T)
    for op in NONCOMM:
        bx, by = D.binary_bound_ulp(op, T)
        for X, rows, c in binary_blocks(op, T):
            for form, (_, which) in FORMS.items():
                # ŷ is the operand the tangent rides on: grid x for d/dx, grid y for d/dy
                yh, tgt = (X[0], X[1]) if which == "x" else (X[1], X[0])
                P, sp, bulp = (c["dx"][rows], c["sx"][rows], bx) if which == "x" else (c["dy"][rows], c["sy"][rows], by)
                loss = expr_loss(op, form)
                ds = srhip.DeviceDataset(ctx, yh[None, :].astype(T), tgt.astype(T))
                s, g, wsum, ok = prog.eval_loss_grad(ds, loss.kind, loss.params)
                what = f"{op} {form} {np.dtype(T).name}"
                assert ok.all() and ctx.last_tree_code() == 0, what
                if op in D.zero_binary():
                    assert g[0] == 0.0
                    continue
                term = P * yh
                bound = np.sum(partial_tol(P, sp, bulp, T, yh) + D.ulp_of(term, T)) + RTOL[np.dtype(T)] * np.abs(term).sum()
                tails.add(f"{op} {form}", check(g[:1], [term.sum()], [bound], what))
    for op in EXPR_UNARY:
        x, d, sp = D.unary_case(op, T)
        keep = (np.abs(d) < 1e6) & np.isfinite(sp)
        r = np.flatnonzero(keep)[np.arange(NROWS) % int(keep.sum())]
        loss = expr_loss(op, None)
        ds = srhip.DeviceDataset(ctx, x[r][None, :].astype(T), np.zeros(NROWS, dtype=T))
        s, g, wsum, ok = prog.eval_loss_grad(ds, loss.kind, loss.params)
        assert ok.all(), op
        term = d[r] * x[r]
        bound = (np.sum(partial_tol(d[r], sp[r], D.unary_bound_ulp(op, T), T, x[r]) + D.ulp_of(term, T))
                 + RTOL[np.dtype(T)] * np.abs(term).sum())
        tails.add(op, check(g[:1], [term.sum()], [bound], f"{op} expression loss {np.dtype(T).name}"))
    tails.flush()


# ---- d. conventions and failure --------------------------------------------------------

def cycled(a):
    a = np.asarray(a, dtype=np.float64)
    return a[np.arange(NROWS) % len(a)]


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
def test_conventions(gpu_ctx, T):
    """The convention table through the engine: the class of every entry is the one written by hand, and a
    finite result equals the oracle's in T."""
    ctx = gpu_ctx
    table = D.conv_unary(T)
    ops = sorted({op for op, _, _ in table})
    X = np.stack([cycled([x for o, x, _ in table if o == op]) for op in ops]).astype(T)
    trees = [D.unary_tree(op, i + 1) for i, op in enumerate(ops)]
    prog = srhip.Program(ctx, srhip.flatten(trees, D.options(), dtype=T), T)
    val, grad, ok = prog.eval_grad_tree_array(srhip.DeviceDataset(ctx, X, np.zeros(NROWS, dtype=T)))
    assert ok.all(), [op for op, k in zip(ops, ok) if not k]  # the value is finite at every convention point
    assert prog.pass_info()["grad_items"] == (len(ops), 0, 0, 0) and ctx.last_tree_code() == 0
    for i, op in enumerate(ops):
        rows = [(x, cls) for o, x, cls in table if o == op]
        _, g_or, okr = D.oracle_unary_d(op, X[i].astype(np.float64), T)
        assert okr
        for r, (x, cls) in enumerate(rows):
            assert D.class_matches(grad[i][r], cls, T), (op, x, cls, grad[i][r])
        fin = np.isfinite(g_or)
        assert np.array_equal(grad[i][fin].astype(np.float64), g_or[fin]), op
        assert np.array_equal(np.isnan(grad[i]), np.isnan(g_or)), op
    tb = D.conv_binary(T)
    for op in sorted({r[0] for r in tb}):
        rows = [r[1:] for r in tb if r[0] == op]
        X = np.stack([cycled([r[0] for r in rows]), cycled([r[1] for r in rows])]).astype(T)
        # each partial alone: op(c0 + x1, x2) (V_AX) and op(x1, c0 + x2) (V_XA)
        trees = [B(op, D.carrier(1), feat(2)), B(op, feat(1), D.carrier(2))]
        prog = srhip.Program(ctx, srhip.flatten(trees, D.options(), dtype=T), T)
        val, grad, ok = prog.eval_grad_tree_array(srhip.DeviceDataset(ctx, X, np.zeros(NROWS, dtype=T)))
        assert ok.all(), op
        info = prog.pass_info()
        assert info["grad_items"] == (2, 0, 0, 0) and info["grad_rest"] == (0, 0, 0, 0), info
        assert info["grad_opset"] == ("BASIC" if op in D.BASIC_BINARY else "FULL"), info
        assert ctx.last_tree_code() == 0
        for j, tree in enumerate(trees):
            _, g_or, okr = D.oracle_grad(tree, X, T)
            assert okr
            for r, row in enumerate(rows):
                cls = row[2 + j]
                if cls == "-":
                    continue
                assert D.class_matches(grad[j][r], cls, T), (op, row, "d/dx" if j == 0 else "d/dy", grad[j][r])
                if np.isfinite(g_or[0][r]):
                    assert float(grad[j][r]) == g_or[0][r], (op, row, grad[j][r], g_or[0][r])


SAFE = {"log": -2.0, "log2": -2.0, "log10": -2.0, "log1p": -2.0, "sqrt": -2.0, "acosh": 0.5}


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
def test_out_of_domain_row_fails_the_tree(gpu_ctx, T):
    """One out-of-domain row per safe operator (and a negative base under a fractional power): did_succeed
    is 0 and every constant of the tree gets NaN, from the program's eval_loss_grad (whose kernel cell is
    asserted) and from eval_loss_grad_batch; a healthy tree of the same batch keeps its gradient."""
    ctx = gpu_ctx
    o = D.options()
    names = list(SAFE) + ["pow"]
    X = np.random.default_rng(9).uniform(1.5, 3.0, (len(names) + 1, NROWS))
    trees = []
    for i, op in enumerate(names):
        X[i, 17 + i] = SAFE.get(op, -2.0)  # one bad row, in the full tile
        trees.append(B("*", Node(val=1.5), D.unary_tree(op, i + 1)) if op != "pow"
                     else B("pow", D.carrier(i + 1), Node(val=0.5)))
    trees.append(B("*", Node(val=1.5), D.unary_tree("square", len(names) + 1)))
    X = X.astype(T)
    y = np.zeros(NROWS, dtype=T)
    flat = srhip.flatten(trees, o, dtype=T)
    with np.errstate(all="ignore"):
        _, _, rok = oracle.eval_loss_batch(flat, X, y, dtype=T)
    L2 = srhip.L2DistLoss()
    prog = srhip.Program(ctx, flat, T)
    s, g, wsum, okp = prog.eval_loss_grad(srhip.DeviceDataset(ctx, X, y), L2.kind, L2.params)
    assert ctx.last_tree_code() == 0
    info = prog.pass_info()  # two constants per tree: one G = 2 item each, shallow, full operator set
    assert info["grad_items"] == (0, len(trees), 0, 0) and info["grad_rest"] == (0, 0, 0, 0), info
    assert info["grad_opset"] == "FULL", info
    assert np.array_equal(okp, rok) and np.isnan(s[:-1]).all() and np.isnan(g[:-2]).all() and np.isfinite(g[-2:]).all()
    losses, grads, ok = srhip.eval_loss_grad_batch(trees, srhip.Dataset(X, y), o)
    assert np.array_equal(ok, rok) and list(ok) == [False] * len(names) + [True]
    for t in range(len(names)):
        assert len(grads[t]) == 2 and np.isnan(grads[t]).all(), (names[t], grads[t])
    assert np.isfinite(grads[-1]).all() and np.all(grads[-1] != 0)
