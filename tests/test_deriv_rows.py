"""The reference side of tests/test_deriv_rows_gpu.py, without a GPU (cases: tests/deriv_row_cases.py): every
case's true partial against the Float64 oracle, the bounds and the one-hot condition, the tree code's
acceptance of every case it is meant to run, and the one-hot identity itself on numpy Float32."""
import numpy as np
import pytest

import deriv_row_cases as R
import derivative_cases as D
import srhip
from srhip.engine import jit_compile

TIDS = dict(ids=lambda T: np.dtype(T).name)
ALL_GROUPS = R.TREE_GROUPS + R.EXTRA_GROUPS


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
@pytest.mark.parametrize("group", ALL_GROUPS)
def test_truth_agrees_with_the_oracle(group, T):
    """Every case's partial along every direction against the Float64 oracle's forward mode on the seeded tree
    (deriv_row_cases.row_reference): within 1e-12·|d| plus the fixture's conditioning. A mis-indexed
    feature, a wrong expected sign or a wrong constant shows here, before any GPU run."""
    o = D.options()
    for p in R.problems(group, T):
        XT = p.X.astype(T)
        for c in p.cases:
            v, Dor, ok, _ = R.row_reference(c.tree, o, XT, T)
            assert ok and np.isfinite(v.astype(T)).all(), (p.name, c.name)  # ŷ is finite in T at every row
            for k, d in enumerate(p.dirs):
                truth = p.truth(c, k)
                sp = p.spread[k] if c.chan[k][0] == "target" else 0.0
                tol = 1e-12 * np.abs(truth) + sp
                bad = np.flatnonzero(~(np.abs(Dor[d - 1] - truth) <= tol))
                assert bad.size == 0, (p.name, c.name, d, bad[:5], Dor[d - 1][bad[:5]], truth[bad[:5]])
        # a spare or pad feature is in no tree
        assert not set(p.dirs) & ({R.PAD_FEATURE} | set(R.SPARE))


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
@pytest.mark.parametrize("group", ALL_GROUPS)
def test_bounds_and_one_hot_condition(group, T):
    """Every bound on the grid is finite; every row's target is finite in T (so a row that is not the isolated
    one contributes 0·ℓ = 0); the isolated rows hold every grid point."""
    for p in R.problems(group, T):
        with np.errstate(over="ignore"):
            assert np.isfinite(p.target.astype(T)).all() and np.isfinite(p.X.astype(T)).all(), p.name
        assert 0 < p.ngrid <= p.n, p.name
        assert p.grid[:, p.ngrid:].sum() == 0 or p.grid.all(), p.name
        for c in p.cases:
            for k in range(len(p.dirs)):
                if c.chan[k][0] == "target":
                    for path in (("interp", "tree") if p.tree_code and T == np.float32 else ("interp",)):
                        b = p.bound(c, k, path, T)
                        assert np.isfinite(b[p.grid[k]]).all() and (b[p.grid[k]] > 0).all(), (p.name, c.name, k, path)
                        assert np.isnan(b[~p.grid[k]]).all()
                else:
                    assert np.isfinite(p.expected_exact(c, k, T)).all(), (p.name, c.name, k)


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
def test_no_grid_point_is_dropped(T):
    """The fourteen operators of the tree code keep every point of their grids; an interpreter-only operator
    loses exactly the points whose partial overflows T or whose conditioning the fixture marks as infinite,
    counted from the fixture alone."""
    fx = D.fixture()
    for op in R.TREE_UNARY:
        x, d, sp, dropped = R.unary_grid(op, T)
        assert dropped == 0 and len(x) == len(fx[f"una/{op}/{D.tname(T)}/x"]) >= 27, op
    for op in R.TREE_BINARY:
        c = D.binary_case(op, T)
        with np.errstate(over="ignore"):
            for k in ("dx", "dy"):
                assert np.isfinite(c[k].astype(T)).all(), (op, k)
        assert np.isfinite(c["sx"]).all() and np.isfinite(c["sy"]).all(), op
        main = R.problems(op, T)[0]
        pairs = set(zip(main.X[0, :main.ngrid], main.X[1, :main.ngrid]))
        assert main.ngrid == len(c["x"]) == len(pairs) == (118 if op == "pow" else 108), op
    total = 0
    for ops in R.unary_groups(True):
        for op in ops:
            pre = f"una/{op}/{D.tname(T)}"
            with np.errstate(over="ignore"):
                marked = int((~np.isfinite(fx[f"{pre}/d"].astype(T)) | ~np.isfinite(fx[f"{pre}/spread"])).sum())
            assert R.unary_grid(op, T)[3] == marked, op
            total += marked
    assert total == (2 if T == np.float32 else 0)  # the two acosh operands next to 1 (INFINITE_SPREAD)
    if T == np.float32:  # pow's rows alternate between its blocks: neighbouring rows differ in `a > 0`
        a = R.problems("pow", T)[0].X[0]
        assert (a[:6:3] > 0).all() and (a[1:6:3] < 0).all() and a[2] == 0


@pytest.mark.parametrize("group", R.TREE_GROUPS)
def test_tree_code_accepts_every_case(group):
    """srhip_jit_compile_deriv compiles every tree of every tree-code problem under the spec the GPU test runs
    (L1, weighted), so none can fall back to the interpreter unnoticed."""
    T = np.float32
    for p in R.problems(group, T):
        assert p.tree_code
        flat = R.flat_of(p, T)
        code, text, offs = jit_compile(flat, deriv=([d - 1 for d in p.dirs], R.NF, True), loss=srhip.L1DistLoss())
        assert sorted(offs) == list(range(len(p.cases))), (p.name, sorted(offs))
    for extra in R.EXTRA_GROUPS:  # and none of the interpreter-only operators
        assert not R.problems(extra, T)[0].tree_code


def test_one_hot_identity_in_float32():
    """For d within 64 ulp of t the Float32 difference d - t is exact, and the one-hot weighted sum of |d - t|
    equals it in three summation orders (forward, reverse, pairwise: each adds exact zeros only)."""
    rng = np.random.default_rng(3)
    n = 293
    t = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(np.float32)
    d = t.copy()
    for i in range(n):
        for _ in range(int(rng.integers(0, 65))):
            d[i] = np.nextafter(d[i], np.float32(np.inf if i % 2 else -np.inf))
    loss = np.abs(d - t)  # Float32
    assert np.array_equal(loss.astype(np.float64), np.abs(d.astype(np.float64) - t.astype(np.float64)))
    assert D.ulp_err(d.astype(np.float64), t.astype(np.float64), np.float32).max() <= 64
    for r in range(n):
        w = np.zeros(n, dtype=np.float32)
        w[r] = 1.0
        terms = w * loss
        fwd = np.float32(0)
        for v in terms:
            fwd = np.float32(fwd + v)
        rev = np.float32(0)
        for v in terms[::-1]:
            rev = np.float32(rev + v)
        pair = np.concatenate([terms, np.zeros(512 - n, dtype=np.float32)])
        while len(pair) > 1:
            pair = pair[0::2] + pair[1::2]
        assert fwd == rev == pair[0] == loss[r], r
