"""Every elementwise loss's per-row VALUE ℓ(u) and DERIVATIVE ℓ'(u) in every kernel family that has its own copy of
the loss bodies, against the independent fixture tests/golden/losses.npz (mpmath; tests/golden/make_loss_golden.py):
one matrix, loss configuration x dtype x family. Bounds: loss_cases.py (nothing fitted to the engine's results).

A loss launch returns only Σ w·ℓ, so one row is isolated with one-hot weights: a dataset has 549 rows (512 + 37) and
16 features, feature f cycles through the grid's finite points from its own start (neighbouring lanes take different
branches), tree f is x_f, y = 0 (a margin loss: y = +1, and y = -1 with the features negated, so a = u exactly and
the seed's factor y is exercised), and w is 1 in one hot row and 0 elsewhere: the call returns the 16 values
ℓ(X[f, hot]) exactly and Σ w = 1. The hot row walks PLANT_ROWS until every point has been hot. A non-finite ℓ is
only ever in the hot row (0·Inf = NaN); every tree must report did_succeed: a non-finite loss does not fail a tree.
The derivative: trees c0 + x_f with c0 = 0, eval_loss_grad returns ∂L/∂c0 = w·ℓ'(u) (the -0 point is left out).

Families, each asserting where it landed (last_kernel_name, pass_info, jit_info, last_tree_code, last_bailed):
  shallow-basic / shallow-full / deep / wide   the interpreters, as test_operator_values_gpu.py (Float32 shallow
                      under SRHIP_TI=1 and 0, bit-identical); targets: eval_loss_targets on a two-column
                      MultiDeviceDataset whose other column holds large garbage; rowsets: eval_loss_rowsets;
  tree-code           the loss tree code: Float32 sr_jit_eval_dlpw in PRECISE and default mode, Float64
                      sr_jit64_eval_dlw (the margin losses have no Float64 routine and must run interpreted).
                      Float32 Periodic points beyond kCwCosMax are in launches of their own: every tree is handed
                      back (last_bailed) and equals the interpreter bit for bit;
  unweighted          the W = false instantiations: every point on 1-row datasets (interpreter and tree code) and
                      through eval_loss_rowsets with one-row samples of an unweighted dataset;
  gradients           grad_kernel, grad_kernel_seg (eval_loss_grad_rowsets), grad_kernel_targets, and the gradient
                      tree code (SRHIP_GJIT=1, distance losses; Periodic rows beyond the range fall back and equal
                      the interpreter bit for bit).
Hot weights 0.25 and 8 on the first launch of every configuration: the unit-weight result scaled, bit for bit,
wherever that is a normal number. The worst err / bound per (loss, dtype, family) goes to numerics.record_tail;
profiles/loss_values_parity.json holds one run's figures.
"""
import numpy as np
import pytest

import loss_cases as C
import numerics
import operator_cases as OC
import srhip
from srhip import Node
from test_derivative_rules_gpu import Tails as _Tails
from test_derivative_rules_gpu import env
from test_operator_values_gpu import CNAME, operand

pytestmark = pytest.mark.gpu

NROWS, NF = C.NROWS, C.NFEAT
TIDS = dict(ids=lambda T: np.dtype(T).name)
CONFIGS = [c[0] for c in C.configs()]
INTERP = ["shallow-basic", "shallow-full", "deep", "wide", "targets", "rowsets"]
TREE_CODE = ["tree-code-precise", "tree-code-default"]
GRAD = ["grad", "grad-seg", "grad-targets", "grad-tree-code"]
FULL_OP = next(o for o in ("atan", "tanh", "erf") if o not in OC.BASIC_UNARY)  # makes a program's opset FULL


class Tails(_Tails):
    def flush(self):
        assert all(v <= 1.0 for v in self.worst.values()), self.worst
        numerics.record_tail("loss_values", dict(path=self.path, dtype=self.T, worst_err_over_bound=self.worst))
        print(f"{self.path} {self.T}: worst err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.items())))


def is_margin(cfg):
    return C.config(cfg)[3] == "margin"


def one_hot(rho, n, weight=1.0):
    w = np.zeros(n)
    w[rho] = weight
    return w


class Family:
    """The 16 trees x_f (c0 + x_f for the gradient families) of one family and dtype, built once; run() is one
    launch and asserts where it landed."""

    def __init__(self, ctx, family, T):
        self.ctx, self.family, self.T = ctx, family, np.dtype(T)
        T = self.T
        self.grad = family.startswith("grad")
        fam = "deep" if family == "deep" else "shallow"
        leaves = [operand(f + 1, fam, NF + 1) for f in range(NF)]
        trees = [OC.B("+", Node(val=0.0), x) for x in leaves] if self.grad else leaves
        if family == "shallow-full":
            trees = trees + [OC.U(FULL_OP, OC.feat(NF + 1))]
        self.nt = len(trees)
        flat = srhip.flatten(trees, OC.options(), dtype=T.type)
        self.tree_code = family in TREE_CODE or family == "grad-tree-code"
        if family in TREE_CODE:
            self.mode = {"SRHIP_JIT": "1", **({"SRHIP_JIT_FAST": "0"} if family.endswith("precise") else {})}
            with env(**self.mode):
                self.prog = srhip.Program(ctx, flat, T.type)
            assert self.prog.jit_info()["ntrees"] == self.nt, self.prog.jit_info()
        elif self.grad:
            self.mode = {"SRHIP_GJIT": "1" if self.tree_code else "0"}
            with env(**self.mode):
                self.prog = srhip.Program(ctx, flat, T.type)
            assert list(np.diff(flat.const_off)) == [1] * self.nt
        else:
            self.mode = {"SRHIP_WIDE": "1"} if family == "wide" else {}
            self.prog = srhip.Program(ctx, flat, T.type, interpreted=True)
        self.interp = None  # the interpreter next to tree code, for the handed-back launches
        if self.tree_code:
            with env(SRHIP_GJIT="0"):
                self.interp = srhip.Program(ctx, flat, T.type, interpreted=not self.grad)

    def dataset(self, X, y, w):
        T = self.T
        if self.family in ("targets", "grad-targets"):  # the other column: large garbage
            junk = np.random.default_rng(3).uniform(-1e30, 1e30, len(y))
            Y = np.stack([junk, y]).astype(T)
            W = None if w is None else np.stack([np.abs(junk) * 1e-30, w]).astype(T)
            return srhip.MultiDeviceDataset(self.ctx, X.astype(T), Y, W)
        return srhip.DeviceDataset(self.ctx, X.astype(T), y.astype(T), None if w is None else w.astype(T))

    def call(self, prog, ds, loss, rows=None):
        """(s, g or None, wsum, ok) of one launch through this family's entry point."""
        k, p, fam = loss.kind, loss.params, self.family
        if fam in ("targets", "grad-targets"):
            tg = np.ones(self.nt, dtype=np.int32)
            if self.grad:
                s, g, ws, ok = prog.eval_loss_grad_targets(ds, k, tg, p)
            else:
                (s, ws, ok), g = prog.eval_loss_targets(ds, k, tg, p), None
            ws = np.asarray(ws)[1]
        elif fam in ("rowsets", "grad-seg"):
            idx = np.tile(np.arange(ds.rows, dtype=np.int64), (self.nt, 1)) if rows is None else rows
            if self.grad:
                s, g, ws, ok = prog.eval_loss_grad_rowsets(ds, k, idx, p)
            else:
                (s, ws, ok), g = prog.eval_loss_rowsets(ds, k, idx, p), None
            ws = np.asarray(ws)
            assert np.all(ws == ws[0])
            ws = ws[0]
        elif self.grad:
            s, g, ws, ok = prog.eval_loss_grad(ds, k, p)
        else:
            (s, ws, ok), g = prog.eval_loss(ds, k, p), None
        cp = lambda v: None if v is None else np.array(v, copy=True)
        return cp(s), cp(g), float(ws), np.array(ok, copy=True).astype(bool)

    def run(self, X, y, w, loss, cfg, handed_back=False, rows=None):
        """One launch: (ℓ per tree, ℓ' per tree or None). Asserts the family's kernel, Σ w and did_succeed."""
        ctx, T, fam = self.ctx, self.T, self.family
        f32 = T == np.float32
        ds = self.dataset(X, y, w)
        res = []
        for ti in (("1", "0") if f32 and fam in ("shallow-basic", "shallow-full") else (None,)):
            with env(**self.mode, **({} if ti is None else {"SRHIP_TI": ti})):
                res.append(self.call(self.prog, ds, loss, rows))
                name, ran, bailed = ctx.last_kernel_name(), ctx.last_tree_code(), ctx.last_bailed()
        s, g, ws, ok = res[0]
        for s2, g2, _, ok2 in res[1:]:
            assert np.array_equal(ok, ok2) and s.tobytes() == s2.tobytes(), "SRHIP_TI=1 and SRHIP_TI=0 differ"
        what = (fam, cfg, T.name, name, ran, bailed)
        assert ok.all(), (what, ok)
        expect_w = float(np.sum(w)) if w is not None else float(len(y) if rows is None else rows.shape[1])
        assert ws == expect_w, (what, ws, expect_w)
        wsfx = "" if w is None else "w"
        if fam in TREE_CODE:
            routine = not (is_margin(cfg) and not f32)  # the margin losses have no Float64 routine
            if routine:  # a handed-back call's last kernel is the interpreter's rerun
                assert name == (f"eval_kernel<{CNAME[T]}>" if handed_back else f"sr_jit_eval_dlp{wsfx}" if f32 else f"sr_jit64_eval_dl{wsfx}"), what
                assert ran == self.nt and bailed == (self.nt if handed_back else 0), what
            else:
                assert ran == 0 and name == f"eval_kernel<{CNAME[T]}>", what
        elif fam == "grad-tree-code":
            if is_margin(cfg):  # no seed routine: the interpreter
                assert ran == 0 and name.startswith("grad_kernel"), what
            elif not handed_back:
                assert ran == self.nt and name == (f"sr_jit_grad_dl{wsfx}" if f32 else f"sr_jit64_grad_dl{wsfx}"), what
        else:
            assert ran == 0, what
            want = {"wide": f"eval_kernel_wide<{CNAME[T]}>", "grad": f"grad_kernel<{CNAME[T]}>",
                    "grad-seg": f"grad_kernel_seg<{CNAME[T]}>", "grad-targets": f"grad_kernel_targets<{CNAME[T]}>"}.get(fam)
            assert name == want if want else name.startswith("eval_kernel"), what
            if not self.grad:
                info = self.prog.pass_info()
                assert info["tree_code"] == 0 and (info["shallow"], info["deep"]) == ((0, self.nt) if fam == "deep" else (self.nt, 0)), info
                if fam in ("shallow-basic", "shallow-full"):
                    assert info["opset"] == ("FULL" if fam == "shallow-full" else "BASIC"), info
        if handed_back and self.interp is not None:  # rerun by the interpreter: its results, bit for bit
            with env(SRHIP_GJIT="0", SRHIP_JIT="0"):
                si, gi, _, oki = self.call(self.interp, ds, loss, rows)
                assert ctx.last_tree_code() == 0
            assert oki.all() and s.tobytes() == si.tobytes() and (g is None or g.tobytes() == gi.tobytes()), what
        return s[:NF], None if g is None else g[:NF]


def check_config(fam, cfg, T, tails, scaled_weights=True):
    """Every point of one configuration through one family, with the one-hot layout of the module docstring."""
    loss = C.loss_of(cfg)
    margin = is_margin(cfg)
    what = f"{fam.family}"
    f32_periodic = np.dtype(T) == np.float32 and C.config(cfg)[1] == "PERIODIC"
    for beyond in (False, True):
        for j, (X, rho, pts) in enumerate(C.launches(cfg, T, derivative=fam.grad, beyond=beyond)):
            handed = beyond and f32_periodic and fam.tree_code
            for ysign in ((1.0, -1.0) if margin else (0.0,)):
                Xs = X * (-1.0 if ysign < 0 else 1.0)
                y = np.full(NROWS, ysign)
                s, g = fam.run(Xs, y, one_hot(rho, NROWS), loss, cfg, handed_back=handed)
                if fam.grad and ysign < 0:  # c0 + (-0) is +0 and a = (+0)·(-1): the +0 point arrives as the -0 point
                    u = C.case(cfg, T)["u"]
                    pts = np.where(u[pts] == 0, np.flatnonzero((u == 0) & np.signbit(u))[0], pts)
                tails.add(cfg, C.check(s, cfg, T, "v", f"{what} y={ysign:g}", pts))
                if g is not None:  # a margin loss's seed is y·L'(a): with y = -1 (a = u still) it is -L'(u)
                    tails.add(cfg + "'", C.check(g * (ysign if margin else 1.0), cfg, T, "d", f"{what} y={ysign:g}", pts))
                if scaled_weights and j == 0 and not beyond:
                    for wt in (0.25, 8.0):
                        sw, gw = fam.run(Xs, y, one_hot(rho, NROWS, wt), loss, cfg)
                        for unit, got in ((s, sw), (g, gw)):
                            if unit is None:
                                continue
                            with np.errstate(all="ignore"):
                                want = unit * wt
                                tiny = float(np.finfo(T).tiny)
                                normal = ~np.isfinite(want) | (want == 0) | ((np.abs(want) >= tiny) & (np.abs(unit) >= tiny))
                                exact = np.isfinite(want.astype(T)) | ~np.isfinite(want)  # the scaled value is in T's range
                            sel = normal & exact
                            assert C.same(got[sel], want[sel]).all(), (what, cfg, wt, got[sel], want[sel])


def configs_of(family, part):
    return [c for c in CONFIGS if is_margin(c) == (part == "margin")]


def every_config(cfgs, tails, body):
    """body(cfg) for every configuration: one that fails does not hide the next; all failures are reported."""
    failed = []
    for cfg in cfgs:
        try:
            body(cfg)
        except AssertionError as e:
            failed.append(str(e)[:400])
    assert not failed, f"{len(failed)} configurations failed:\n" + "\n".join(failed)
    tails.flush()


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("part", ["distance", "margin"])
@pytest.mark.parametrize("family", INTERP + TREE_CODE)
def test_loss_values(gpu_ctx, family, part, T):
    if family == "tree-code-default" and np.dtype(T) == np.float64:
        family = "tree-code-precise"  # Float64 has one mode: the parametrisation keeps the cell, the run is the same
    fam = Family(gpu_ctx, family, T)
    tails = Tails(f"values {family} {part}", T)
    every_config(configs_of(family, part), tails, lambda cfg: check_config(fam, cfg, T, tails))


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("part", ["distance", "margin"])
@pytest.mark.parametrize("family", GRAD)
def test_loss_derivatives(gpu_ctx, family, part, T):
    fam = Family(gpu_ctx, family, T)
    tails = Tails(f"derivatives {family} {part}", T)
    every_config(configs_of(family, part), tails, lambda cfg: check_config(fam, cfg, T, tails))


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("family", ["shallow-basic", "tree-code-precise", "grad"])
def test_unweighted_single_rows(gpu_ctx, family, T):
    """The W = false instantiations: every point on 1-row datasets without weights (Σ w is the row count, 1)."""
    fam = Family(gpu_ctx, family, T)
    tails = Tails(f"unweighted {family}", T)
    f32 = np.dtype(T) == np.float32

    def body(cfg):
        loss, margin = C.loss_of(cfg), is_margin(cfg)
        for beyond in (False, True):
            for X, rho, pts in C.launches(cfg, T, derivative=fam.grad, nrows=1, beyond=beyond):
                handed = beyond and f32 and fam.tree_code
                s, g = fam.run(X, np.full(1, 1.0 if margin else 0.0), None, loss, cfg, handed_back=handed)
                tails.add(cfg, C.check(s, cfg, T, "v", f"unweighted {family}", pts))
                if g is not None:
                    tails.add(cfg + "'", C.check(g, cfg, T, "d", f"unweighted {family}", pts))

    every_config(CONFIGS, tails, body)


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("family", ["rowsets", "grad-seg"])
def test_unweighted_one_row_samples(gpu_ctx, family, T):
    """eval_loss_rowsets / eval_loss_grad_rowsets on an unweighted dataset whose rows are the grid itself (every
    feature the same column), tree f scored on the one row 16 j + f: no row with a non-finite ℓ is in another
    tree's sample."""
    fam = Family(gpu_ctx, family, T)
    tails = Tails(f"unweighted one-row samples {family}", T)

    def body(cfg):
        loss, margin = C.loss_of(cfg), is_margin(cfg)
        c = C.case(cfg, T)
        hot = C.hot_points(cfg, T, derivative=fam.grad)
        u = c["u"][hot]
        X = np.vstack([np.tile(u, (NF, 1)), np.ones((1, len(u)))])
        for h0 in range(0, len(u), NF):
            at = (h0 + np.arange(NF)) % len(u)
            s, g = fam.run(X, np.full(len(u), 1.0 if margin else 0.0), None, loss, cfg, rows=at.astype(np.int64)[:, None])
            tails.add(cfg, C.check(s, cfg, T, "v", family, hot[at]))
            if g is not None:
                tails.add(cfg + "'", C.check(g, cfg, T, "d", family, hot[at]))

    every_config(CONFIGS, tails, body)
