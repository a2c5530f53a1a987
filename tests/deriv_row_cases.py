"""Per-row ∂ŷ/∂x of srhip_eval_loss_deriv against tests/golden/derivatives.npz: the cases shared by
tests/test_deriv_rows.py (CPU) and tests/test_deriv_rows_gpu.py. Importable without a GPU.

The call returns channel sums only. With one-hot weights (1.0 at row r, 0.0 elsewhere) in every channel,
the L1 loss and the target t_r = fl_T(true partial at row r), channel 1 + k's sum is |d_r - t_r| bit for bit:
the subtraction is exact (Sterbenz) while d_r is within a factor 2 of t_r, 1·ℓ = ℓ, 0·ℓ = 0 for a finite ℓ,
and adding zeros is exact in any order (the lanes' sums, the wave sum, the Float64 finalize). So one call per
row hands back the engine's own per-row error, from the forward-mode interpreter and from the reverse-mode
tree code alike.

A dataset has one target column per direction, shared by every tree of the program. So a Problem is a
dataset (X, directions, one true partial per direction and row) and the trees scored against it; a tree's
channel is either
  "target": its partial is the column's truth, held to a bound in ulps of T, or
  "exact":  its partial is a value T holds and the engine must produce without error (0 for a feature the
            tree does not read, ±1, ±2, an operand of `*`, the -0.0-scaled tangent), so the channel's sum
            must EQUAL |fl_T(e_r) - t_r| computed in T, whatever the column's truth is.
Cases that need another truth on the same feature (a constant operand, a flipped sign, a second
contribution) are Problems of their own or read a copy of the feature.

Bounds (nothing fitted to the engine's results), per isolated grid row:
  partial_tol(P, spread, bulp, T) as in test_derivative_rules_gpu (bulp ulp_T(P) + 4 spread) + 0.5 ulp_T(t) for
  rounding the target (+ Problem.extra: the rounding of a sum of two contributions).
  bulp is the fixture's count (derivative_cases.unary_bound_ulp / binary_bound_ulp) where the path runs the rule
  that count describes: the interpreter always, the tree code for neg abs square cube exp + - *. Where the
  tree code's reverse rule is its own, bulp is TREE_CODE_ULP below: the roundings of jit_grad.cpp emit_reverse
  counted at 1 ulp per v_rcp_f32 and 0.5 ulp per v_mul_f32, plus the forward value's bar (numerics.py:
  + - * / and sqrt correctly rounded, 0.5 ulp; a transcendental 4 ulp) where the rule reuses it and the
  routine's stated bar where it calls one.
Rows: NROWS = 293 (a full 256-row tile and a partial one). A unary operator's feature holds its grid, then
in-domain fill (rows_with_fill). Every one of the 293 rows is isolated once: grid rows are held to a bound,
every row to the exact channels. A binary operator's features repeat its grid pairs, so every row is a grid point; pow mixes its
three blocks row by row (lanes of one wave differ in `a > 0`).
"""
import dataclasses
import functools

import numpy as np

import derivative_cases as D
import srhip
from srhip import Node
from srhip.interface import _seed_features
from test_gradients import grad_spread

NROWS = D.NROWS
NF = 9           # features of every problem: 1..4 the operands, 5 the deep pad's, 6..9 spare directions
PAD_FEATURE = 5  # read by the deep variant's pad only, never a direction
SPARE = (6, 7, 8, 9)  # read by no tree: the extra directions of a 5-direction call (two tangent groups)
TREE_UNARY = ("neg", "abs", "square", "cube", "exp", "sin", "cos", "log", "sqrt")  # jit_grad.cpp kGradUops
TREE_BINARY = ("+", "-", "*", "/", "pow")                                            # kGradBops
EXACT_BINARY = ("+", "-", "*")  # partials ±1 or an operand: the fixture's bound is 0

# Float32 tree code, rules of its own (jit_grad.cpp emit_reverse), in ulps of the partial. g is the incoming
# adjoint (the seed 1 here; its multiply is counted all the same).
TREE_CODE_ULP = {
    ("/", "x"): 1.5,    # g·rcp(b): v_rcp_f32 1 + v_mul_f32 0.5
    ("/", "y"): 2.5,    # (g·rcp(b))·q: the 1.5 above + the forward quotient q (correctly rounded) 0.5 + v_mul_f32 0.5
    ("log", "x"): 1.5,  # s·rcp(a·s)·g, s = 2^±64 or 1 (both scalings exact): v_rcp_f32 1 + v_mul_f32 0.5
    ("sqrt", "x"): 2.5,  # rcp(s)·0.5·g: the forward root s (correctly rounded) 0.5 + v_rcp_f32 1 + two v_mul_f32 1.0
    ("sin", "x"): 2.5,  # g·cos a: the FAST cos routine or sincos_pd_f32's factor, both stated <= 2 ulp (device_ops.h) + v_mul_f32 0.5
    ("cos", "x"): 2.5,  # -g·sin a: as sin
    # ("pow", "x"): g·(b·safe_pow(a, b - 1)): the fixture's oracle_err_ulp (the oracle runs b·pow(a, b - 1) in T
    #     with a libm pow: the rounding of b - 1 and of the product b·pow) + the PRECISE pow routine 4 + v_mul_f32 0.5
    ("pow", "y"): 9.0,  # g·(f·log a): the forward power f (PRECISE routine) 4 + the PRECISE log routine 4 + two v_mul_f32 1.0
}


def B(op, l, r):
    return D.options().make_binary(op, l, r)


def feat(f):
    return Node(feature=f)


def scaled(f, c=1.0):
    """x_f * c: a computed operand whose value is x_f (c = 1.0)."""
    return B("*", feat(f), Node(val=c))


def partial_tol(P, spread, bulp, T):
    """bulp ulp_T(P) + 4 spread: test_derivative_rules_gpu.partial_tol at a tangent of 1."""
    return bulp * D.ulp_of(P, T) + 4.0 * spread


def row_reference(tree, o, X, T):
    """(ŷ [n], ∂ŷ/∂x [nfeat, n], ok, spread of ∂ŷ/∂x [nfeat, n]) from the Float64 oracle's forward mode on
    the `x + (-0.0)`-seeded tree (constants rounded to T), as test_deriv_loss_gpu.row_reference."""
    binops = tuple(o.binary_operators)
    plus = binops.index("+") + 1
    aug, seeds = _seed_features(tree, plus, None)
    v, g, ok, _, sg = grad_spread(aug, o, X, T)
    seeds = np.asarray(seeds)
    nfeat, n = X.shape
    Dx, S = np.zeros((nfeat, n)), np.zeros((nfeat, n))
    for f in range(1, nfeat + 1):
        m = seeds == f
        if m.any():
            Dx[f - 1] = g[m].sum(axis=0)
            S[f - 1] = sg[m].sum(axis=0)
    return v, Dx, bool(ok), S


def tree_code_ulp(op, which, T):
    """bulp of the Float32 tree code's rule for operator `op`, partial `which` ("x" / "y")."""
    if (op, which) == ("pow", "x"):
        return float(D.fixture()["bin/pow/f32/oracle_err_ulp"][0]) + 4.0 + 0.5
    if (op, which) in TREE_CODE_ULP:
        return TREE_CODE_ULP[(op, which)]
    return interp_ulp(op, which, T)


def interp_ulp(op, which, T):
    if op in D.binary_ops():
        return float(D.binary_bound_ulp(op, T)[0 if which == "x" else 1])
    return D.unary_bound_ulp(op, T)


@dataclasses.dataclass
class Case:
    name: str
    op: str       # the operator the case is recorded under
    tree: Node
    chan: list    # per direction: ("target", which) or ("exact", e [n] float64)


@dataclasses.dataclass
class Problem:
    name: str
    ops: tuple          # per direction: the operator whose partial the column holds, or None
    X: np.ndarray       # [NF, n] float64
    dirs: list          # 1-based features
    target: np.ndarray  # [ndir, n] float64: the column's true partial (the fixture's on grid rows)
    P: np.ndarray       # [ndir, n] the fixture partial whose ulps scale the bound (|P| = |target| but for a sum)
    spread: np.ndarray  # [ndir, n] the fixture's conditioning of P
    extra: np.ndarray   # [ndir, n] absolute terms added to the bound
    grid: np.ndarray    # [ndir, n] bool: the row's target is a fixture value (it has a bound)
    ngrid: int          # rows 0 .. ngrid-1 hold every grid point once (every row is isolated)
    cases: list
    tree_code: bool     # every tree is within the tree code's operator set

    @property
    def n(self):
        return self.X.shape[1]

    def bound(self, case, k, path, T):
        """[n] bound of |d - t| on channel k of a "target" case (NaN off the grid). path: "interp" / "tree"."""
        kind, which = case.chan[k]
        assert kind == "target"
        op = self.ops[k]
        bulp = tree_code_ulp(op, which, T) if path == "tree" else interp_ulp(op, which, T)
        tol = partial_tol(self.P[k], self.spread[k], bulp, T) + self.extra[k] + 0.5 * D.ulp_of(self.target[k], T)
        return np.where(self.grid[k], tol, np.nan)

    def expected_exact(self, case, k, T):
        """[n] the channel's sum with row r isolated, when the tree's partial is exactly e: |fl_T(e) - t| in T."""
        kind, e = case.chan[k]
        assert kind == "exact"
        return np.abs(np.asarray(e, dtype=T) - self.target[k].astype(T)).astype(np.float64)

    def truth(self, case, k):
        """[n] the case's own true partial along direction k, as float64."""
        kind, e = case.chan[k]
        return self.target[k] if kind == "target" else np.asarray(e, dtype=np.float64)


def _fill_features(X, seed):
    """Features nobody set: in [0.5, 1.5], Float32-rounded."""
    rng = np.random.default_rng(seed)
    for f in range(X.shape[0]):
        if np.isnan(X[f]).all():
            X[f] = rng.uniform(0.5, 1.5, X.shape[1]).astype(np.float32).astype(np.float64)
    assert np.isfinite(X).all()
    return X


def zeros(n):
    return np.zeros(n)


def exact(e):
    return ("exact", np.asarray(e, dtype=np.float64))


def const(v):
    return Node(val=float(v))


def minus0(f):
    """x_f + (-0.0): x_f bit for bit, computed."""
    return B("+", feat(f), const(-0.0))


# ---- unary operators --------------------------------------------------------------------------------

def unary_grid(op, T):
    """(x, d, spread, dropped): the operator's grid without the points whose partial is not finite in T or
    whose conditioning is not finite (the two acosh operands the fixture's generator marks)."""
    x, d, sp = D.unary_case(op, T)
    with np.errstate(over="ignore"):
        keep = np.isfinite(d.astype(T)) & np.isfinite(sp)
    return x[keep], d[keep], sp[keep], int((~keep).sum())


def unary_groups(extra):
    """Operators four by four (four directions per program): the tree code's, or the interpreter-only rest."""
    ops = [o for o in D.unary_ops() if o not in TREE_UNARY] if extra else list(TREE_UNARY)
    return [tuple(ops[i:i + 4]) for i in range(0, len(ops), 4)]


def unary_problem(ops, T, name, seed=900):
    """Per operator i (feature i + 1, direction i): op(x), op(x·1.0), op(x + (-0.0)). The other channels of a
    tree are exactly 0."""
    n, nd = NROWS, len(ops)
    X = np.full((NF, n), np.nan)
    target, spread, grid = np.zeros((nd, n)), np.zeros((nd, n)), np.zeros((nd, n), dtype=bool)
    o = D.options()
    cases = []
    for i, op in enumerate(ops):
        x, d, sp, _ = unary_grid(op, T)
        X[i] = D.rows_with_fill(x, op, T, seed + i)
        target[i, :len(x)], spread[i, :len(x)], grid[i, :len(x)] = d, sp, True
    _fill_features(X, seed - 1)
    for i, op in enumerate(ops):
        f = i + 1
        chan = [("target", "x") if k == i else exact(zeros(n)) for k in range(nd)]
        for what, operand in (("x", feat(f)), ("x*1", scaled(f)), ("x+-0", minus0(f))):
            cases.append(Case(f"{op}({what})", op, o.make_unary(op, operand), chan))
        # the fill rows' target: the Float64 oracle's partial (finite; such a row is never held to a bound)
        ng = int(grid[i].sum())
        if ng < n:
            target[i, ng:] = row_reference(cases[-3].tree, o, X.astype(T), T)[1][i, ng:]
    assert np.isfinite(target).all()
    return Problem(name, tuple(ops), X, list(range(1, nd + 1)), target, target.copy(), spread, np.zeros((nd, n)), grid,
                   int(grid.sum(axis=1).max()), cases, all(op in TREE_UNARY for op in ops))


# ---- binary operators -------------------------------------------------------------------------------

def binary_rows(op, T, blocks, n):
    """(fixture index of each of n rows, the fixture arrays, number of distinct points): the blocks' pairs
    interleaved block by block (rows alternate between the blocks), repeated to n rows."""
    c = D.binary_case(op, T)
    idx = np.flatnonzero(np.isin(c["block"], blocks))
    rank = np.zeros(len(idx), dtype=int)
    for b in blocks:
        m = c["block"][idx] == b
        rank[m] = np.arange(int(m.sum()))
    idx = idx[np.lexsort((c["block"][idx], rank))]
    return idx[np.arange(n) % len(idx)], c, len(idx)


def binary_main(op, T, n=NROWS):
    """Features 1 = a, 2 = b, 3 = w > 0, 4 = a again. Directions [1, 2, 3, 4]: dx, dy, 0, dx + 1.
    op(a, b) as V_XX, V_AX, V_XA, V_AT, V_TA (test_derivative_rules_gpu.shape), and op(x4, b) + x4: two
    contributions to one direction block."""
    blocks = [0, 1, 2] if op == "pow" else [0]
    rows, c, npts = binary_rows(op, T, blocks, n)
    X = np.full((NF, n), np.nan)
    X[0], X[1], X[3] = c["x"][rows], c["y"][rows], c["x"][rows]
    X[2] = np.random.default_rng(77).uniform(0.5, 2.0, n).astype(np.float32).astype(np.float64)
    _fill_features(X, 78)
    dx, dy, sx, sy = c["dx"][rows], c["dy"][rows], c["sx"][rows], c["sy"][rows]
    target = np.stack([dx, dy, zeros(n), dx + 1.0])
    P = np.stack([dx, dy, zeros(n), dx])
    spread = np.stack([sx, sy, zeros(n), sx])
    # the sum of the two contributions rounds once, in the engine's binade, which may be the one above the
    # target's: 1 ulp_T(dx + 1)
    extra = np.stack([zeros(n), zeros(n), zeros(n), D.ulp_of(dx + 1.0, T)])
    z = exact(zeros(n))
    main = [("target", "x"), ("target", "y"), z, z]
    if op in EXACT_BINARY:  # the partials are values T holds: equality
        main = [exact(dx), exact(dy), z, z]
    shapes = [
        ("XX", B(op, feat(1), feat(2))),
        ("AX", B(op, scaled(1), feat(2))),
        ("XA", B(op, feat(1), scaled(2))),
        # the right operand needs more stack: emitted first (V_AT); x2·1.0 + x3·(-0.0) == x2 bit for bit
        ("AT", B(op, scaled(1), B("+", scaled(2), scaled(3, -0.0)))),
        ("TA", B(op, B("+", scaled(1), scaled(3, -0.0)), scaled(2))),
    ]
    cases = [Case(f"{op} {v}", op, t, main) for v, t in shapes]
    both = [z, exact(dy) if op in EXACT_BINARY else ("target", "y"), z,
            exact(dx + 1.0) if op in EXACT_BINARY else ("target", "x")]
    cases.append(Case(f"{op} XX+x", op, B("+", B(op, feat(4), feat(2)), feat(4)), both))
    grid = np.ones((4, n), dtype=bool)
    return Problem(f"{op} main", (op, op, None, op), X, [1, 2, 3, 4], target, P, spread, extra, grid, npts, cases, True)


def one_direction(p, k):
    """Problem p along direction k alone, with the trees that have a target there: the other operand is a
    feature that is no direction (no reverse code, no tangent seed)."""
    cases = [Case(c.name + f" dir x{p.dirs[k]}", c.op, c.tree, [c.chan[k]]) for c in p.cases[:3]]
    s = slice(k, k + 1)
    return Problem(f"{p.name} dir x{p.dirs[k]}", p.ops[s], p.X, p.dirs[s], p.target[s], p.P[s], p.spread[s], p.extra[s],
                   p.grid[s], p.ngrid, cases, p.tree_code)


def binary_const(op, T):
    """A constant operand, block 0 (a full product, so (a, c) and (c, b) are grid points at every row):
    op(a, c), op(a·1.0, c) along a (V_XC, V_AC) and op(c', b), op(c', b·1.0) along b (V_CX, V_CA)."""
    n = NROWS
    rows, c, npts = binary_rows(op, T, [0], n)
    look = {(float(x), float(y)): i for i, (x, y) in enumerate(zip(c["x"], c["y"]))}
    X = np.full((NF, n), np.nan)
    X[0], X[1] = c["x"][rows], c["y"][rows]
    _fill_features(X, 79)
    ys, xs = sorted(set(X[1])), sorted(set(X[0]))
    cy, cx = ys[len(ys) // 2], xs[len(xs) // 2]
    at_a = np.array([look[(float(a), cy)] for a in X[0]])
    at_b = np.array([look[(cx, float(b))] for b in X[1]])
    target = np.stack([c["dx"][at_a], c["dy"][at_b]])
    spread = np.stack([c["sx"][at_a], c["sy"][at_b]])
    z = exact(zeros(n))
    ta = [exact(target[0]) if op in EXACT_BINARY else ("target", "x"), z]
    tb = [z, exact(target[1]) if op in EXACT_BINARY else ("target", "y")]
    cases = [Case(f"{op} XC", op, B(op, feat(1), const(cy)), ta), Case(f"{op} AC", op, B(op, scaled(1), const(cy)), ta),
             Case(f"{op} CX", op, B(op, const(cx), feat(2)), tb), Case(f"{op} CA", op, B(op, const(cx), scaled(2)), tb)]
    return Problem(f"{op} const", (op, op), X, [1, 2], target, target.copy(), spread, np.zeros((2, n)),
                   np.ones((2, n), dtype=bool), npts, cases, True)


# ---- sign chains, roots, direction order ---------------------------------------------------------------

SIGN_INNER = (("cos", "log"), ("sin", "sqrt"), ("exp", "cube"), "/", "pow")  # the inner operators of the chains


def _sign_operands(inner, T):
    """(X, per operand feature (true partial, spread, operator, which), tree of the inner value per operand,
    distinct grid rows). Two unary operators: x1, x2 hold their grids within |x| <= 1e6 and |d| <= 1e30 (the
    chain's value stays finite), repeated. A binary one: x1, x2 hold its pairs (pow: block 0). x3, x4 in [-3, 3]."""
    n = NROWS
    o = D.options()
    X = np.full((NF, n), np.nan)
    per, ngrid = [], 0
    if isinstance(inner, tuple):
        for i, op in enumerate(inner):
            x, d, sp, _ = unary_grid(op, T)
            keep = np.flatnonzero((np.abs(x) <= 1e6) & (np.abs(d) <= 1e30))
            r = keep[np.arange(n) % len(keep)]
            X[i] = x[r]
            per.append((d[r], sp[r], op, "x", o.make_unary(op, feat(i + 1))))
            ngrid = max(ngrid, len(keep))
    else:
        rows, c, ngrid = binary_rows(inner, T, [0], n)
        X[0], X[1] = c["x"][rows], c["y"][rows]
        per = [(c["dx"][rows], c["sx"][rows], inner, "x", B(inner, feat(1), feat(2))),
               (c["dy"][rows], c["sy"][rows], inner, "y", None)]
    X[2:4] = np.random.default_rng(81).uniform(-3, 3, (2, n)).astype(np.float32).astype(np.float64)
    _fill_features(X, 82)
    return X, per, ngrid


def sign_problems(inner, T):
    """neg(f), neg(neg(x)), neg(x) - x against the targets -f', 1, -2, and x3 - (x4 - f) against +f', 1, -1,
    with f = op(x1), op(x2) for two unary operators or op(x1, x2) for a binary one: the sign flag through
    share_adj and dir_add into every kind of reverse rule, and the interpreter's tangents."""
    n = NROWS
    X, per, ngrid = _sign_operands(inner, T)
    o = D.options()
    z, one = exact(zeros(n)), np.ones(n)
    unary = isinstance(inner, tuple)
    name = "+".join(inner) if unary else inner
    P = np.stack([per[0][0], per[1][0], zeros(n), zeros(n)])
    sp = np.stack([per[0][1], per[1][1], zeros(n), zeros(n)])
    ops = (per[0][2], per[1][2], None, None)
    tgt = [("target", per[0][3]), ("target", per[1][3])]
    grid = np.ones((4, n), dtype=bool)
    zero = np.zeros((4, n))
    flipped, chain = [], []
    for i in range(2):
        f = per[i][4]
        if f is None:
            continue
        own = [tgt[k] if (k == i or not unary) else z for k in range(2)]
        flipped.append(Case(f"neg({name}) #{i}", per[i][2], o.make_unary("neg", f), own + [z, z]))
        chain.append(Case(f"x3-(x4-{name}) #{i}", per[i][2], B("-", feat(3), B("-", feat(4), f)),
                          own + [exact(one), exact(-one)]))
    flipped.append(Case("neg(x)-x", "neg", B("-", o.make_unary("neg", feat(3)), feat(3)), [z, z, exact(-2 * one), z]))
    flipped.append(Case("neg(neg(x))", "neg", o.make_unary("neg", o.make_unary("neg", feat(4))), [z, z, z, exact(one)]))
    t1 = np.stack([-P[0], -P[1], -2 * one, one])
    t2 = np.stack([P[0], P[1], one, -one])
    return [Problem(f"signs flipped {name}", ops, X, [1, 2, 3, 4], t1, P, sp, zero, grid, ngrid, flipped, True),
            Problem(f"signs chain {name}", ops, X, [1, 2, 3, 4], t2, P, sp, zero, grid, ngrid, chain, True)]


def root_problems(T):
    """x1 / x3 under the directions [3, 1] and [1, 3] (channel k follows dir[k]), and the trees without an
    operator: x1 (a direction: exactly 1 there, 0 along x3), x2 (no direction), a constant (no reverse code)."""
    n = NROWS
    rows, c, npts = binary_rows("/", T, [0], n)
    X = np.full((NF, n), np.nan)
    X[0], X[2] = c["x"][rows], c["y"][rows]
    _fill_features(X, 83)
    per = {1: (c["dx"][rows], c["sx"][rows], "x"), 3: (c["dy"][rows], c["sy"][rows], "y")}
    z = exact(zeros(n))
    out = []
    for dirs in ([3, 1], [1, 3]):
        target = np.stack([per[d][0] for d in dirs])
        spread = np.stack([per[d][1] for d in dirs])
        cases = [Case(f"x1/x3 dirs {dirs}", "/", B("/", feat(1), feat(3)), [("target", per[d][2]) for d in dirs]),
                 Case(f"x1 dirs {dirs}", "root", feat(1), [exact(np.ones(n)) if d == 1 else z for d in dirs]),
                 Case(f"x2 dirs {dirs}", "root", feat(2), [z, z]),
                 Case(f"const dirs {dirs}", "root", const(2.5), [z, z])]
        out.append(Problem(f"roots {dirs}", ("/", "/"), X, dirs, target, target.copy(), spread, np.zeros((2, n)),
                           np.ones((2, n), dtype=bool), npts, cases, True))
    return out


# ---- the groups the tests are parametrised over --------------------------------------------------------

TREE_GROUPS = [f"unary-{i}" for i in range(len(unary_groups(False)))] + list(TREE_BINARY) + [f"signs-{i}" for i in range(len(SIGN_INNER))] + ["roots"]
EXTRA_GROUPS = [f"extra-{i}" for i in range(len(unary_groups(True)))]


@functools.lru_cache(maxsize=None)
def problems(group, T):
    """The problems of one group, built once per dtype and left unchanged."""
    if group.startswith(("unary-", "extra-")):
        extra = group.startswith("extra-")
        return [unary_problem(unary_groups(extra)[int(group.split("-")[1])], T, group)]
    if group.startswith("signs-"):
        return sign_problems(SIGN_INNER[int(group.split("-")[1])], T)
    if group == "roots":
        return root_problems(T)
    main = binary_main(group, T)
    return [main, one_direction(main, 0), one_direction(main, 1), binary_const(group, T)]


def padded(tree):
    """The tree inside one that needs 5 stack slots (the deep variant). The pad reads a feature that is no
    direction and is added with `+`: every ∂ŷ/∂x_d is unchanged."""
    return B("+", tree, D.pad_tree(PAD_FEATURE))


def directions(p, five):
    """The call's directions: the problem's, or those plus spare features (read by no tree) up to five."""
    return list(p.dirs) + (list(SPARE)[:5 - len(p.dirs)] if five else [])


def flat_of(p, T, deep=False):
    return srhip.flatten([padded(c.tree) if deep else c.tree for c in p.cases], D.options(), dtype=T)
