"""Per-row ∂ŷ/∂x of both paths of srhip_eval_loss_deriv — the forward-mode interpreter (grad_kernel_deriv<T>:
shallow, deep, two tangent groups, wide) and the reverse-mode tree code (sr_jit_deriv_w) — against the mpmath
fixture tests/golden/derivatives.npz, one isolated row per call (cases, the one-hot identity and every bound:
tests/deriv_row_cases.py; nothing is fitted to the engine's results). Each (path, dtype, operator) records its
worst err / bound through numerics.record_tail("deriv_rows", ...); profiles/deriv_rows_parity.json holds a
run's figures."""
import numpy as np
import pytest

import deriv_row_cases as R
import derivative_cases as D
import numerics
from srhip import constants as K
from srhip.engine import MultiDeviceDataset, Program
from test_derivative_rules_gpu import Tails, env

pytestmark = pytest.mark.gpu

L1, HUBER = K.LOSS["L1"], K.LOSS["HUBER"]
F32 = np.float32
TIDS = dict(ids=lambda T: np.dtype(T).name)
CNAME = {np.dtype(np.float32): "float", np.dtype(np.float64): "double"}
VARIANTS = ("shallow", "deep", "groups", "wide")


class RowTails(Tails):
    def flush(self):
        assert all(v <= 1.0 for v in self.worst.values()), self.worst
        numerics.record_tail("deriv_rows", dict(path=self.path, dtype=self.T, worst_err_over_bound=self.worst))
        print(f"{self.path} {self.T}: worst err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.items())))


def columns(p, dirs, T):
    """Y [1 + ndir, n]: y = 0 and fl_T(true partial) per direction (0 for a spare direction)."""
    Y = np.zeros((1 + len(dirs), p.n), dtype=T)
    Y[1:1 + len(p.dirs)] = p.target.astype(T)
    return Y


def isolated_rows(ctx, prog, p, dirs, rows, T, kernel, ncode):
    """One eval_loss_deriv per row r of `rows` with W[k] = e_r in every channel, L1: sums [len(rows), ntrees,
    1 + ndir]. Asserts the kernel, the tree-code count, Σw = 1, the flags and a finite channel 0 at every call."""
    X, Y = p.X.astype(T), columns(p, dirs, T)
    out = np.empty((len(rows), len(p.cases), 1 + len(dirs)))
    for i, r in enumerate(rows):
        W = np.zeros_like(Y)
        W[:, r] = 1.0
        sums, wsum, ok = prog.eval_loss_deriv(MultiDeviceDataset(ctx, X, Y, W), L1, [d - 1 for d in dirs])
        assert ctx.last_kernel_name() == kernel and ctx.last_tree_code() == ncode, (p.name, ctx.last_kernel_name())
        assert np.array_equal(wsum, np.ones(1 + len(dirs))), wsum
        assert ok.all(), (p.name, r, [c.name for c, k in zip(p.cases, ok) if not k])
        assert np.isfinite(sums[:, 0]).all(), (p.name, r, sums[:, 0])
        out[i] = sums
    return out


def check_rows(p, sums, rows, path, T, tails):
    """Every "target" channel within its bound at every isolated grid row; every "exact" channel equal to
    |fl_T(e) - t| at every isolated row; a spare direction's channel exactly 0."""
    rows = np.asarray(rows)
    for t, c in enumerate(p.cases):
        for k in range(len(p.dirs)):
            got = sums[:, t, 1 + k]
            what = f"{p.name}: {c.name} x{p.dirs[k]} {path} {np.dtype(T).name}"
            if c.chan[k][0] == "exact":
                want = p.expected_exact(c, k, T)[rows]
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (what, rows[bad[:5]], got[bad[:5]], want[bad[:5]])
                tails.add(c.op, 0.0)
                continue
            bound = p.bound(c, k, "tree" if path == "tree code" else "interp", T)[rows]
            on = ~np.isnan(bound)
            bad = np.flatnonzero(on & ~(got <= bound))
            assert bad.size == 0, (what, rows[bad[:5]], got[bad[:5]], bound[bad[:5]], p.X[:4, rows[bad[:5]]])
            if on.any():
                tails.add(c.op, float(np.max(got[on] / bound[on])))
        assert not sums[:, t, 1 + len(p.dirs):].any(), (p.name, c.name, "a spare direction")


@pytest.mark.parametrize("group", R.TREE_GROUPS)
def test_rows_tree_code(gpu_ctx, group):
    """The reverse rules of jit_grad.cpp's dv mode, per operator and per row: adjoints routed to feature leaves
    (give / dir_add), the sign flag through share_adj, opreg's re-read feature operand, the sin / cos factor,
    DIV's flipped sign on the divisor, POW's two rules with lanes that differ in a > 0, the three root cases and
    the direction order."""
    tails = RowTails("tree code", F32)
    for p in R.problems(group, F32):
        prog = Program(gpu_ctx, R.flat_of(p, F32), F32, interpreted=True, deriv_tree_code=True)
        rows = np.arange(p.n)
        sums = isolated_rows(gpu_ctx, prog, p, p.dirs, rows, F32, "sr_jit_deriv_w", len(p.cases))
        check_rows(p, sums, rows, "tree code", F32, tails)
    tails.flush()


@pytest.mark.parametrize("T", D.DTYPES, **TIDS)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("group", R.TREE_GROUPS + R.EXTRA_GROUPS)
def test_rows_interpreter(gpu_ctx, group, variant, T):
    """The same cases and isolation in the forward-mode interpreter: the shallow variants, the deep one (each tree
    plus a feature-only pad over a feature that is no direction), a 5-direction call (two tangent groups; the
    spare directions are in no tree: exactly 0) and the wide variant (SRHIP_WIDE=1)."""
    tails = RowTails(f"interpreter {variant}", T)
    kernel = f"grad_kernel_{'wide_' if variant == 'wide' else ''}deriv<{CNAME[np.dtype(T)]}>"
    for p in R.problems(group, T):
        prog = Program(gpu_ctx, R.flat_of(p, T, deep=variant == "deep"), T, interpreted=True)
        dirs = R.directions(p, five=variant == "groups")
        rows = np.arange(p.n)
        with env(**({"SRHIP_WIDE": "1"} if variant == "wide" else {})):
            sums = isolated_rows(gpu_ctx, prog, p, dirs, rows, T, kernel, 0)
        if variant == "deep":
            assert prog.pass_info()["grad_items"][3] >= 1, prog.pass_info()
        if variant == "groups":
            assert len(dirs) == 5
        check_rows(p, sums, rows, "interpreter", T, tails)
    tails.flush()


def full_sums(ctx, p, T, kind, params, weights, tree_code):
    X, Y = p.X.astype(T), columns(p, p.dirs, T)
    W = np.ones_like(Y) if weights else None
    prog = Program(ctx, R.flat_of(p, T), T, interpreted=True, deriv_tree_code=tree_code)
    sums, wsum, ok = prog.eval_loss_deriv(MultiDeviceDataset(ctx, X, Y, W), kind, [d - 1 for d in p.dirs], params)
    assert ok.all() and np.array_equal(wsum, np.full(1 + len(p.dirs), float(p.n)))
    return sums, ctx.last_kernel_name(), ctx.last_tree_code()


@pytest.mark.parametrize("tree_code", [True, False], ids=["tree code", "interpreter"])
@pytest.mark.parametrize("group", ["/", "pow"])
def test_unweighted_equals_unit_weights(gpu_ctx, group, tree_code):
    """Over all 293 rows (every one a grid point), L1 and Huber(1): W = None and W ≡ 1 give bit-identical sums.
    Tree code: sr_jit_deriv against sr_jit_deriv_w, whose emit_channel differs by one multiply by the weight.
    Interpreter: grad_kernel.h's kGradLossDeriv branch differs by `if constexpr (W) l = wv[e] * l;` alone (the
    row count gives both one row group, and -ffp-contract=off keeps the product apart from the sum). And the L1
    sum of a "target" channel stays within the sum of its rows' bounds."""
    p = R.problems(group, F32)[0]
    ncode = len(p.cases) if tree_code else 0
    names = ("sr_jit_deriv", "sr_jit_deriv_w") if tree_code else ("grad_kernel_deriv<float>",) * 2
    tails = RowTails("L1 sum, " + ("tree code" if tree_code else "interpreter"), F32)
    for kind, params in ((L1, None), (HUBER, [1.0])):
        a, na, ca = full_sums(gpu_ctx, p, F32, kind, params, False, tree_code)
        b, nb, cb = full_sums(gpu_ctx, p, F32, kind, params, True, tree_code)
        assert (na, nb) == names and ca == cb == ncode
        assert a.tobytes() == b.tobytes(), (kind, a, b)
        if kind != L1:
            continue
        for t, c in enumerate(p.cases):
            for k in range(len(p.dirs)):
                if c.chan[k][0] == "target":
                    bound = p.bound(c, k, "tree" if tree_code else "interp", F32).sum()
                    print(f"{c.name} x{p.dirs[k]}: L1 sum {a[t, 1 + k]:.3e} bound {bound:.3e}")
                    assert a[t, 1 + k] <= bound, (c.name, k, a[t, 1 + k], bound)
                    tails.add(c.op, a[t, 1 + k] / bound)
    tails.flush()


@pytest.mark.parametrize("tree_code", [True, False], ids=["tree code", "interpreter"])
def test_last_row_and_padding(gpu_ctx, tree_code):
    """The tile edge, the first row of the partial tile and the last row (255, 256, 292 of 293), and rows 2047 and
    2048 of 2049, which lie in different row groups (a weighted tile gives a workgroup 1024 rows:
    test_deriv_tree_code_gpu.py's docstring): the rows past the last one are masked, the row groups' partials
    are summed, and the isolated row still comes back bit for bit."""
    path = "tree code" if tree_code else "interpreter"
    tails = RowTails(f"edges, {path}", F32)
    for p, rows in ((R.problems("/", F32)[0], [255, 256, 292]), (R.binary_main("/", F32, n=2049), [2047, 2048])):
        prog = Program(gpu_ctx, R.flat_of(p, F32), F32, interpreted=True, deriv_tree_code=tree_code)
        sums = isolated_rows(gpu_ctx, prog, p, p.dirs, rows, F32, "sr_jit_deriv_w" if tree_code else "grad_kernel_deriv<float>",
                             len(p.cases) if tree_code else 0)
        if p.n == 2049:
            assert gpu_ctx.last_loss_launch()["nrg"] >= 2, gpu_ctx.last_loss_launch()
        check_rows(p, sums, rows, path, F32, tails)
    tails.flush()
