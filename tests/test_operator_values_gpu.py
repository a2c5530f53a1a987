"""Every operator's VALUE in every kernel family that has its own copy of the operator bodies, against the
independent fixture tests/golden/operators.npz (exact rational arithmetic and mpmath;
tests/golden/make_operator_golden.py): one matrix, operator x dtype x family.

Every dataset has 549 rows (512 + 37: one full tile of every family's row tile plus a partial one), and the
rows cycle through the operator's grid in grid order (from another start for every feature), so neighbouring
lanes hold tiny next to huge operands and take different branches of a routine; each point lands in at least two
lanes and row slots. One feature per operator (two per binary block), one tree per operator (per block).

Families, each asserting where it landed (last_kernel_name, pass_info, jit_info, last_tree_code, last_bailed):
  shallow-basic / shallow-full   the shallow interpreter, `Program(..., interpreted=True).eval_tree_array`; Float32
                                 under SRHIP_TI=1 and SRHIP_TI=0, bit-identical to each other. The threaded
                                 interpreter hands a tile back to the C++ dispatch inside the kernel (the host cannot
                                 see it); it takes the BASIC operators only, so the shallow-full cell runs the C++
                                 dispatch in both settings;
  deep                           the deep interpreter kernel: the same node over `x - Z`, Z a feature-only balanced
                                 subtree of stack need 5 whose value is exactly +0.0 (x - (+0.0) == x bit for bit,
                                 -0.0 included: checked with the oracle on the CPU below);
  wide                           SRHIP_WIDE=1: eval_kernel_wide;
  tree-code                      the per-row output tree code, SRHIP_JIT=1 at program creation (sr_jit_out_d /
                                 sr_jit64_out), every tree taken; bit-identical to the shallow interpreter's outputs.
The binary operators run in the `x1 ∘ x2` form in every family and in the eight other operand forms the compiler
emits (XC CX AX XA AC CA AT TA, the tree shapes of test_derivative_rules_gpu.shape) in the interpreter.
did_succeed: every entry of the fixture's failure tables planted in one row of a column of in-domain fill (the
row varies over lanes, the full tile and the partial one); the neighbouring still-finite operand, planted the
same way, succeeds with the fixture's value.

The loss tree code (sr_jit_eval_dlp / sr_jit64_eval_dl) returns sums only: see the section on it below (PRECISE, the
default with its FAST exp / sin / cos and `/`, without the packed and hand-scheduled bodies, and the memory-constant
code sr_jit_eval_dlm with every value of either side of every block as the constant operand), with the failure tables planted through each mode.
The gradient tree code's own derivative rules (SRHIP_GJIT=1) are the last section, on the grids of
tests/golden/derivatives.npz.

Bounds: operator_cases.py (the project's per-operator bars; nothing fitted to the engine's results). The worst
err / bound per (operator, dtype, family) goes to numerics.record_tail; profiles/operator_values_parity.json
holds one run's figures.
"""
import numpy as np
import pytest

import numerics
import operator_cases as C
import oracle
import srhip
from test_derivative_rules_gpu import Tails as _Tails
from test_derivative_rules_gpu import env, shape

pytestmark = pytest.mark.gpu

NROWS = C.NROWS
TIDS = dict(ids=lambda T: np.dtype(T).name)
FAMILIES = ["shallow-basic", "shallow-full", "deep", "wide", "tree-code"]
CNAME = {np.dtype(np.float32): "float", np.dtype(np.float64): "double"}
MAX_BLOCKS = 8  # binary blocks per launch: 16 features and the pad's
PLANT_ROWS = (0, 63, 64, 130, 255, 256, 511, 512, 548)  # lanes, wave and tile borders, the partial tile


class Tails(_Tails):
    def flush(self):
        assert all(v <= 1.0 for v in self.worst.values()), self.worst
        numerics.record_tail("operator_values", dict(path=self.path, dtype=self.T, worst_err_over_bound=self.worst))
        print(f"{self.path} {self.T}: worst err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.worst.items())))


# ---- running one batch in one family ---------------------------------------------------------

def run(ctx, family, trees, X, T, basic):
    """eval_tree_array of `trees` in `family`: (out, ok), copied. Asserts where the batch landed. In the
    interpreter families a Float32 batch runs under SRHIP_TI=1 and 0, and the two must agree bit for bit."""
    T = np.dtype(T)
    flat = srhip.flatten(trees, C.options(), dtype=T.type)
    ds = srhip.DeviceDataset(ctx, X.astype(T), np.zeros(X.shape[1], dtype=T))
    nt = len(trees)
    if family == "tree-code":
        with env(SRHIP_JIT="1"):
            prog = srhip.Program(ctx, flat, T.type)
        assert prog.jit_info()["ntrees"] == nt, prog.jit_info()
        out, ok = (np.array(v, copy=True) for v in prog.eval_tree_array(ds))
        assert ctx.last_tree_code() == nt and ctx.last_bailed() == 0
        assert ctx.last_kernel_name() == ("sr_jit_out_d" if T == np.float32 else "sr_jit64_out"), ctx.last_kernel_name()
        return out, ok
    prog = srhip.Program(ctx, flat, T.type, interpreted=True)
    wide = family == "wide"
    res = []
    for ti in (("1", "0") if T == np.float32 else ("1",)):
        with env(SRHIP_TI=ti, **({"SRHIP_WIDE": "1"} if wide else {})):
            res.append(tuple(np.array(v, copy=True) for v in prog.eval_tree_array(ds)))
            name = ctx.last_kernel_name()
        assert name == f"eval_kernel{'_wide' if wide else ''}<{CNAME[T]}>", name
        assert ctx.last_tree_code() == 0
    info = prog.pass_info()
    assert info["tree_code"] == 0 and (info["shallow"], info["deep"]) == ((0, nt) if family == "deep" else (nt, 0)), info
    if family in ("shallow-basic", "shallow-full"):
        assert info["opset"] == ("BASIC" if basic else "FULL"), info
    out, ok = res[0]
    for o2, k2 in res[1:]:
        assert np.array_equal(ok, k2) and out.tobytes() == o2.tobytes(), "SRHIP_TI=1 and SRHIP_TI=0 differ"
    return out, ok


def is_basic(ops):
    return all(op in C.BASIC_UNARY or op in C.BASIC_BINARY for op in ops)


def operand(feature, family, pad_feature):
    """x_feature, in the deep family as x - Z with Z = +0.0 from a subtree of stack need 5."""
    return C.B("-", C.feat(feature), C.zero_pad(pad_feature)) if family == "deep" else C.feat(feature)


def pad_column(seed=0):
    return np.random.default_rng(seed).uniform(0.5, 1.5, NROWS).astype(np.float32).astype(np.float64)


def rows_of(case, idx):
    return {k: (None if v is None else v[idx]) for k, v in case.items() if k not in ("a", "b")}


def test_the_deep_operand_is_the_grid_value():
    """x - Z == x bit for bit with Z = +0.0 (the oracle, on the CPU), -0.0 and the extremes included."""
    for T in C.DTYPES:
        x = np.concatenate([C.unary_case("neg", T)["x"], C.unary_case("exp", T)["x"]])
        X = np.stack([x, np.linspace(0.5, 1.5, len(x))]).astype(T)
        flat = srhip.flatten([operand(1, "deep", 2), C.zero_pad(2)], C.options(), dtype=T)
        out, ok = oracle.eval_trees(flat, X, dtype=T)
        assert ok.all() and C.same_bits(out[0], X[0]).all() and C.same_bits(out[1], np.zeros(len(x), dtype=T)).all()


# ---- a, b, d, e, f: the unary operators ------------------------------------------------------

def unary_batches(family):
    basic = [o for o in C.unary_ops() if o in C.BASIC_UNARY]
    if family == "shallow-basic":
        return [basic]
    ops = C.unary_ops()  # the FULL batch holds every operator, the BASIC ones again
    return [ops[:15], ops[15:]]


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_unary_values(gpu_ctx, family, T):
    ctx = gpu_ctx
    tails = Tails(f"unary {family}", T)
    for ops in unary_batches(family):
        nf = len(ops) + 1
        X = np.empty((nf, NROWS))
        idx = {}
        for i, op in enumerate(ops):
            X[i], idx[op] = C.cycled(C.unary_case(op, T)["x"], start=7 * i)
        X[nf - 1] = pad_column()
        trees = [C.U(op, operand(i + 1, family, nf)) for i, op in enumerate(ops)]
        out, ok = run(ctx, family, trees, X, T, basic=family == "shallow-basic")
        assert ok.all(), [op for op, k in zip(ops, ok) if not k]
        if family == "tree-code":  # the project's stated property, here at the edges
            ref, rok = run(ctx, "shallow-full", trees, X, T, basic=all(o in C.BASIC_UNARY for o in ops))
            assert rok.all() and out.tobytes() == ref.tobytes(), [op for i, op in enumerate(ops) if out[i].tobytes() != ref[i].tobytes()]
        for i, op in enumerate(ops):
            tails.add(op, C.check_values(out[i], op, T, rows_of(C.unary_case(op, T), idx[op]), f"{op} {np.dtype(T).name} {family}"))
    tails.flush()


# ---- a, b, d, e, f: the binary operators, x1 ∘ x2 ----------------------------------------------

def binary_batches(family, T):
    """[[(op, block index)]]: the BASIC operators' blocks and the others', at most MAX_BLOCKS per launch."""
    groups = [[(op, k) for op in C.binary_ops() if (op in C.BASIC_BINARY) == b for k in range(len(C.binary_blocks(op, T)))]
              for b in (True, False)]
    if family == "shallow-basic":
        groups = groups[:1]
    return [g[i:i + MAX_BLOCKS] for g in groups for i in range(0, len(g), MAX_BLOCKS)]


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_binary_values(gpu_ctx, family, T):
    ctx = gpu_ctx
    tails = Tails(f"binary {family}", T)
    for batch in binary_batches(family, T):
        nf = 2 * len(batch) + 1
        X = np.empty((nf, NROWS))
        idx = []
        for i, (op, k) in enumerate(batch):
            blk = C.binary_blocks(op, T)[k]
            _, ix = C.cycled(blk["x"], start=5 * i)
            X[2 * i], X[2 * i + 1] = blk["x"][ix], blk["y"][ix]
            idx.append(ix)
        X[nf - 1] = pad_column()
        trees = [C.B(op, operand(2 * i + 1, family, nf), C.feat(2 * i + 2)) for i, (op, k) in enumerate(batch)]
        basic = all(op in C.BASIC_BINARY for op, _ in batch)
        out, ok = run(ctx, family, trees, X, T, basic=basic)
        assert ok.all(), [b for b, k in zip(batch, ok) if not k]
        if family == "tree-code":
            ref, rok = run(ctx, "shallow-full", trees, X, T, basic=basic)
            assert rok.all() and out.tobytes() == ref.tobytes(), [b for i, b in enumerate(batch) if out[i].tobytes() != ref[i].tobytes()]
        for i, (op, k) in enumerate(batch):
            tails.add(op, C.check_values(out[i], op, T, rows_of(C.binary_blocks(op, T)[k], idx[i]),
                                         f"{op} block {k} {np.dtype(T).name} {family}"))
    tails.flush()


# ---- c. the binary operand forms of the interpreter --------------------------------------------

FORMS = ["V_XC", "V_CX", "V_AX", "V_XA", "V_AC", "V_CA", "V_AT", "V_TA"]  # V_XX is test_binary_values' form
NONCOMM = ("-", "/", "pow", "mod", "max", "min", "greater")


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("form", FORMS)
def test_binary_operand_forms(gpu_ctx, form, T):
    """The non-commutative operators in the eight other operand forms compile.cpp emits, on every block: a
    constant operand takes each value of its side of the block in turn (one tree each, at most 60 per launch),
    the other side cycles; computed operands are x · 1.0 (and + w · (-0.0), w > 0): the grid value bit for bit."""
    ctx = gpu_ctx
    tails = Tails(f"binary form {form}", T)
    const_y, const_x = form in ("V_XC", "V_AC"), form in ("V_CX", "V_CA")
    for op in NONCOMM:
        for k, blk in enumerate(C.binary_blocks(op, T)):
            na, nb = len(blk["a"]), len(blk["b"])
            ia, ib = np.arange(NROWS) % na, np.arange(NROWS) % nb
            if not (const_x or const_y):  # both sides from the data: cycle through the product
                _, ix = C.cycled(blk["x"], start=3 * k)
                ia, ib = ix // nb, ix % nb
            X = np.stack([blk["a"][ia], blk["b"][ib], pad_column(k + 1)])
            consts = list(blk["b"]) if const_y else list(blk["a"]) if const_x else [None]
            trees = [shape(form, op, None if c is None else float(c))[0] for c in consts]
            for t0 in range(0, len(trees), 60):
                out, ok = run(ctx, "shallow-full", trees[t0:t0 + 60], X, T, basic=op in C.BASIC_BINARY)
                assert ok.all(), (op, k, form)
                for j, o in enumerate(out):
                    c = t0 + j
                    at = (ia * nb + c) if const_y else (c * nb + ib) if const_x else (ia * nb + ib)
                    tails.add(op, C.check_values(o, op, T, rows_of(blk, at), f"{op} block {k} {form} const {consts[c]!r} {np.dtype(T).name}"))
    tails.flush()


# ---- i. did_succeed ------------------------------------------------------------------------------

def fill_value(op, T):
    """(an in-domain operand of the grid, its index): the middle of the grid."""
    c = C.unary_case(op, T)
    i = len(c["x"]) // 2
    return c["x"][i], i


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_planted_failures(gpu_ctx, family, T):
    """Every entry of the failure tables: a column of in-domain fill with the bad operand in one row fails its
    tree; the same column with the neighbouring still-finite operand succeeds, with the fixture's value in that
    row and the grid's in the others. The verdicts are the hand-written ones (the oracle agrees with them on the
    CPU: test_operator_values.py)."""
    ctx = gpu_ctx
    fu, fb = C.fail_unary(T), C.fail_binary(T)
    assert len(fu) >= 30 and len(fb) >= 25
    if family == "shallow-basic":  # the BASIC opset (the only batches the threaded interpreter takes)
        fu, fb = [e for e in fu if e[0] in C.BASIC_UNARY], [e for e in fb if e[0] in C.BASIC_BINARY]
        assert len(fu) >= 8 and len(fb) >= 8
    per = 8  # entries per launch: two columns each (the binary ones four), and the pad's
    for e0 in range(0, len(fu), per):
        part = fu[e0:e0 + per]
        nf = 2 * len(part) + 1
        X = np.empty((nf, NROWS))
        trees, rows = [], []
        for i, (op, bad, good, val) in enumerate(part):
            r = PLANT_ROWS[(e0 + i) % len(PLANT_ROWS)]
            X[2 * i], X[2 * i + 1] = fill_value(op, T)[0], fill_value(op, T)[0]
            X[2 * i, r], X[2 * i + 1, r] = bad, good
            trees += [C.U(op, operand(2 * i + 1, family, nf)), C.U(op, operand(2 * i + 2, family, nf))]
            rows.append(r)
        X[nf - 1] = pad_column()
        out, ok = run(ctx, family, trees, X, T, basic=is_basic(p[0] for p in part))
        assert list(ok) == [False, True] * len(part), [(p[:3], bool(ok[2 * i]), bool(ok[2 * i + 1])) for i, p in enumerate(part)]
        for i, (op, bad, good, val) in enumerate(part):
            what = f"{op} at {good!r} (next to {bad!r}) {np.dtype(T).name} {family}"
            C.check_values(out[2 * i + 1][rows[i]:rows[i] + 1], op, T, C.point_case(op, T, val), what)
            c, j = C.unary_case(op, T), fill_value(op, T)[1]
            rest = np.delete(out[2 * i + 1], rows[i])
            C.check_values(rest, op, T, rows_of(c, np.full(NROWS - 1, j)), what + ": the fill")
    per = 4
    for e0 in range(0, len(fb), per):
        part = fb[e0:e0 + per]
        nf = 4 * len(part) + 1
        X = np.empty((nf, NROWS))
        trees, rows = [], []
        for i, (op, bx, by, gx, gy, val) in enumerate(part):
            r = PLANT_ROWS[(e0 + i + 3) % len(PLANT_ROWS)]
            X[4 * i], X[4 * i + 1], X[4 * i + 2], X[4 * i + 3] = gx, gy, gx, gy  # the fill is the good pair itself
            X[4 * i, r], X[4 * i + 1, r] = bx, by
            trees += [C.B(op, operand(4 * i + 1, family, nf), C.feat(4 * i + 2)), C.B(op, operand(4 * i + 3, family, nf), C.feat(4 * i + 4))]
            rows.append(r)
        X[nf - 1] = pad_column()
        out, ok = run(ctx, family, trees, X, T, basic=is_basic(p[0] for p in part))
        assert list(ok) == [False, True] * len(part), [(p[:5], bool(ok[2 * i]), bool(ok[2 * i + 1])) for i, p in enumerate(part)]
        for i, (op, bx, by, gx, gy, val) in enumerate(part):
            case = C.point_case(op, T, val)
            case = {k: (None if v is None else np.repeat(v, NROWS)) for k, v in case.items()}
            C.check_values(out[2 * i + 1], op, T, case, f"{op} at ({gx!r}, {gy!r}) {np.dtype(T).name} {family}")


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_conventions(gpu_ctx, family, T):
    """The convention table (signed zeros, ties, mod's sign, pow's special cases) through the engine: the value
    written by hand next to the reference's line, bit for bit."""
    ctx = gpu_ctx
    conv = C.conventions(T)
    for kind in ("una", "bin"):
        ops = [op for op in (C.unary_ops() if kind == "una" else C.binary_ops()) if any(c[0] == op for c in conv)]
        if family == "shallow-basic":
            ops = [op for op in ops if is_basic([op])]
        for o0 in range(0, len(ops), MAX_BLOCKS):
            part = ops[o0:o0 + MAX_BLOCKS]
            nf = 2 * len(part) + 1
            X = np.empty((nf, NROWS))
            trees, want = [], []
            for i, op in enumerate(part):
                ent = [c for c in conv if c[0] == op]
                ix = (np.arange(NROWS) + i) % len(ent)
                X[2 * i] = np.array([e[1] for e in ent])[ix]
                X[2 * i + 1] = np.array([1.0 if e[2] is None else e[2] for e in ent])[ix]
                want.append(np.array([e[3] for e in ent])[ix].astype(T))
                trees.append(C.U(op, operand(2 * i + 1, family, nf)) if kind == "una"
                             else C.B(op, operand(2 * i + 1, family, nf), C.feat(2 * i + 2)))
            X[nf - 1] = pad_column()
            out, ok = run(ctx, family, trees, X, T, basic=is_basic(part))
            assert ok.all(), part
            for i, op in enumerate(part):
                if not C.is_exact(op):  # pow: the value within its bar, a zero with the written sign
                    w64 = want[i].astype(np.float64)
                    C.check_values(out[i], op, T, dict(x=X[2 * i], y=X[2 * i + 1], hi=w64, lo=np.zeros(NROWS), rn=None), f"{op} conventions {family}")
                    same = (want[i] != 0) | C.same_bits(out[i], want[i])
                else:
                    same = C.same_bits(out[i], want[i])
                assert same.all(), (op, family, X[2 * i][~same][:4], X[2 * i + 1][~same][:4], out[i][~same][:4], want[i][~same][:4])


# ---- g, h: the loss tree code --------------------------------------------------------------------
# The loss tree code returns only sums, so the trees are op(x_i) - x_j with y = 0 and L2, where x_j holds the
# interpreter's own per-row output of op(x_i) (the construction of test_constant_divisor_is_ieee_exact). The
# subtraction is exact at that distance, so a PRECISE body gives a sum of exactly 0 and a FAST exp / sin / cos
# body at most Σ (2 ulp_T(x_j))² (1 + RTOL) (test_margin_losses_gpu.RTOL: the Float32 row sum's allowance).
# A batch builds its two programs once and runs them on every dataset.

FAST_UNARY = ("exp", "sin", "cos")  # what the FAST region admits among the unary operators (jit_info's nfast)
GUARD = 15.0  # inside every FAST guard (|x| < 16 for exp, far below 105615 for the trigonometric reduction)
DIV_LO, DIV_HI = 2.0 ** -44, 2.0 ** 44  # strictly inside the packed division's [2^-45, 2^45] and above 2^-50
LOSS_MODES = {"precise": {"SRHIP_JIT_FAST": "0"}, "default": {}, "plain-bodies": {"SRHIP_JIT_MANUAL": "0", "SRHIP_JIT_PACKED": "0"},
              "memory-constants": {}}
L2 = srhip.L2DistLoss()


def fast_ops_of(mode, T):
    """The operators whose trees jit_info counts as FAST in this mode (the FAST `/` is a packed body)."""
    if np.dtype(T) != np.float32 or mode == "precise":
        return ()
    return FAST_UNARY + (("/",) if mode in ("default", "memory-constants") else ())


def guarded_rows(inside, k):
    """Row -> point index: the first full tile (512 rows) cycles through the points inside every FAST guard, so
    the FAST bodies are what computes it before a redo makes the tree sticky-PRECISE; the partial tile holds the
    k-th slice of 37 of the others (past the guards, past 105615, tiny and huge). A set of points with nothing
    inside cycles as it is."""
    ins, outs = np.flatnonzero(inside), np.flatnonzero(~inside)
    if not len(ins):
        return (37 * k + np.arange(NROWS)) % len(inside)
    idx = ins[np.arange(NROWS) % len(ins)]
    if len(outs):
        idx[512:] = outs[(37 * k + np.arange(NROWS - 512)) % len(outs)]
    return idx


def nslices(inside):
    return max(1, -(-int(np.sum(~inside)) // 37)) if inside.any() else 1


class LossBatch:
    """The trees `inner[i] - x_(nf1 + i + 1)` as loss tree code in one mode, next to the interpreted `inner`."""

    def __init__(self, ctx, T, mode, inner, names, nf1):
        self.ctx, self.T, self.mode, self.names, self.nf1 = ctx, np.dtype(T), mode, list(names), nf1
        T = self.T
        self.interp = srhip.Program(ctx, srhip.flatten(inner, C.options(), dtype=T.type), T.type, interpreted=True)
        trees = [C.B("-", t, C.feat(nf1 + i + 1)) for i, t in enumerate(inner)]
        self.memc = mode == "memory-constants"
        with env(SRHIP_JIT="1", **LOSS_MODES[mode]):
            self.prog = srhip.Program(ctx, srhip.flatten(trees, C.options(), dtype=T.type), T.type, varying_constants=self.memc)
        info = self.prog.jit_info()
        self.nfast = sum(op in fast_ops_of(mode, T) for op in names)
        assert info["ntrees"] == len(names) and info["nfast"] == self.nfast, (info, names, mode)

    def outputs(self, X1):
        out, ok = (np.array(v, copy=True) for v in self.interp.eval_tree_array(
            srhip.DeviceDataset(self.ctx, X1.astype(self.T), np.zeros(NROWS, dtype=self.T))))
        assert self.ctx.last_tree_code() == 0 and ok.all(), self.names
        return out

    def sums(self, X1, xj):
        """(Σ (inner - x_j)² per tree, ok) through the loss tree code; asserts that it ran."""
        ctx, T = self.ctx, self.T
        X2 = np.vstack([X1, np.asarray(xj, dtype=np.float64)])
        with env(SRHIP_JIT="1", **LOSS_MODES[self.mode]):
            s, wsum, ok = self.prog.eval_loss(srhip.DeviceDataset(ctx, X2.astype(T), np.zeros(NROWS, dtype=T)), L2.kind, L2.params)
            name, ran, bailed = ctx.last_kernel_name(), ctx.last_tree_code(), ctx.last_bailed()
        want = "sr_jit64_eval_dl" if T == np.float64 else "sr_jit_eval_dlm" if self.memc else "sr_jit_eval_dlp"
        assert name == want and ran == len(self.names) and bailed == 0 and wsum == NROWS, (name, want, ran, bailed)
        return np.array(s, copy=True), np.array(ok, copy=True)

    def bound(self, i, xj_row):
        """0 for a PRECISE body; the FAST exp / sin / cos bodies: Σ (2 ulp_T(x_j))² (1 + RTOL). This is a bound on
        the row sum, all the loss code returns: one row alone could be some tens of ulps off below it (549 rows
        share it); a wrong body is far outside (a lost sign is 10^14 times the bound), an error of a few ulps
        in one lane is what the per-row families and the PRECISE mode's exact 0 are for."""
        from test_margin_losses_gpu import RTOL

        if self.nfast and self.names[i] in FAST_UNARY:
            return float(np.sum((2.0 * C.ulp_of(np.asarray(xj_row, dtype=np.float64), self.T)) ** 2)) * (1 + RTOL[self.T])
        return 0.0

    def check(self, X1, worst):
        out = self.outputs(X1)
        s, ok = self.sums(X1, out)
        assert ok.all(), [op for op, k in zip(self.names, ok) if not k]
        for i, op in enumerate(self.names):
            b = self.bound(i, out[i])
            assert 0.0 <= s[i] <= b, (op, self.mode, s[i], b)
            worst[op] = max(worst.get(op, 0.0), float(s[i]) / b if b else 0.0)


def loss_modes(T, memc=False):
    return [m for m in LOSS_MODES if m != "memory-constants" or (memc and np.dtype(T) == np.float32)]


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("mode", loss_modes(np.float64))
def test_loss_tree_code_unary(gpu_ctx, mode, T):
    tails = Tails(f"loss tree code {mode} unary", T)
    ops = C.unary_ops()
    for o0 in range(0, len(ops), 8):
        part = ops[o0:o0 + 8]
        batch = LossBatch(gpu_ctx, T, mode, [C.U(op, C.feat(i + 1)) for i, op in enumerate(part)], part, len(part))
        xs = [C.unary_case(op, T)["x"] for op in part]
        for k in range(max(nslices(np.abs(x) <= GUARD) for x in xs)):
            batch.check(np.stack([x[guarded_rows(np.abs(x) <= GUARD, k)] for x in xs]), tails.worst)
    tails.flush()


def div_inside(x, y):
    ax, ay = np.abs(x), np.abs(y)
    return (ax >= DIV_LO) & (ax <= DIV_HI) & (ay >= DIV_LO) & (ay <= DIV_HI)


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("mode", loss_modes(np.float64))
def test_loss_tree_code_binary(gpu_ctx, mode, T):
    """x1 ∘ x2 - x3 on every block: every binary body of the loss tree code is held to the interpreter's bits
    (`/` too: the packed and FAST divisions are IEEE-exact inside their range and redone outside it). The first
    full tile holds only pairs with both operands in [2^-44, 2^44], the others follow in the partial tile."""
    tails = Tails(f"loss tree code {mode} binary", T)
    cells = [(op, k) for op in C.binary_ops() for k in range(len(C.binary_blocks(op, T)))]
    for c0 in range(0, len(cells), 5):
        part = cells[c0:c0 + 5]
        blks = [C.binary_blocks(op, T)[k] for op, k in part]
        names = [op for op, _ in part]
        batch = LossBatch(gpu_ctx, T, mode, [C.B(op, C.feat(2 * i + 1), C.feat(2 * i + 2)) for i, op in enumerate(names)], names, 2 * len(part))
        ins = [div_inside(b["x"], b["y"]) for b in blks]
        for k in range(max(nslices(m) for m in ins)):
            rows = [guarded_rows(m, k) for m in ins]
            batch.check(np.stack([b[key][r] for b, r in zip(blks, rows) for key in ("x", "y")]), tails.worst)
    tails.flush()


@pytest.mark.parametrize("side", ["constant-right", "constant-left"])
def test_loss_tree_code_memory_constants(gpu_ctx, side):
    """The memory-constant code (varying_constants=True; Float32 only: Float64 tree code holds its constants as
    literals): x ∘ c and c ∘ x with c each value of that side of a block, the other side cycling with the pairs
    inside the division's range first. sr_jit_eval_dlm is asserted; sums exactly 0."""
    T = np.float32
    tails = Tails(f"loss tree code memory-constants {side}", T)
    right = side == "constant-right"
    for op in C.binary_ops():
        for blk in C.binary_blocks(op, T):
            var, consts = (blk["a"], blk["b"]) if right else (blk["b"], blk["a"])
            assert len(consts) <= 60  # every constant of the side: one tree each, one launch
            inner = [C.B(op, C.feat(1), srhip.Node(val=float(c))) if right else C.B(op, srhip.Node(val=float(c)), C.feat(1)) for c in consts]
            names = [op] * len(consts)
            batch = LossBatch(gpu_ctx, T, "memory-constants", inner, names, 1)
            inside = (np.abs(var) >= DIV_LO) & (np.abs(var) <= DIV_HI)
            for k in range(nslices(inside)):
                batch.check(var[guarded_rows(inside, k)][None, :], tails.worst)
    tails.flush()


# ---- i. did_succeed through the loss tree code -----------------------------------------------------

def plant_loss(ctx, T, mode, inner_of, entries, ncol, tails):
    """entries: [(op, bad operands (ncol), good operands (ncol), fill operands (ncol))]. Per entry two trees over
    their own columns: fill with the bad operand(s) in one row, and with the good one(s). x_j is the
    interpreter's output of the good column (0 in the bad row of the bad tree). The bad tree fails with a NaN
    sum, the good one succeeds within the mode's bound."""
    per = 4
    for e0 in range(0, len(entries), per):
        part = entries[e0:e0 + per]
        names = [e[0] for e in part for _ in (0, 1)]
        nf1 = 2 * ncol * len(part)
        inner = [inner_of(op, ncol * j + 1) for j, op in enumerate(names)]
        batch = LossBatch(ctx, T, mode, inner, names, nf1)
        X = np.empty((nf1, NROWS))
        Xg = np.empty((nf1, NROWS))
        rows = []
        for i, (op, bad, good, fill) in enumerate(part):
            r = PLANT_ROWS[(e0 + i + 5) % len(PLANT_ROWS)]
            rows.append(r)
            for c in range(ncol):
                for tree, val in ((0, bad[c]), (1, good[c])):
                    f = (2 * i + tree) * ncol + c
                    X[f], Xg[f] = fill[c], fill[c]
                    X[f, r], Xg[f, r] = val, good[c]
        out = batch.outputs(Xg)  # every column holds the good operand: finite everywhere
        xj = out.astype(np.float64)
        for i, r in enumerate(rows):
            xj[2 * i, r] = 0.0
        s, ok = batch.sums(X, xj)
        assert list(ok) == [False, True] * len(part), (mode, [(e[:3], bool(ok[2 * i]), bool(ok[2 * i + 1])) for i, e in enumerate(part)])
        for i, (op, *_) in enumerate(part):
            assert np.isnan(s[2 * i]), (op, mode, s[2 * i])  # a failed tree's sum is NaN
            b = batch.bound(2 * i + 1, out[2 * i + 1])
            assert 0.0 <= s[2 * i + 1] <= b, (op, mode, s[2 * i + 1], b)
            tails.add(op, float(s[2 * i + 1]) / b if b else 0.0)


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("mode", loss_modes(np.float64))
def test_planted_failures_loss_tree_code(gpu_ctx, mode, T):
    """Every failure-table entry through eval_loss in each loss mode: did_succeed is the hand-written verdict, a
    failed tree reports a NaN sum, the still-finite neighbour's tree succeeds."""
    tails = Tails(f"planted failures, loss tree code {mode}", T)
    fu = [(op, (bad,), (good,), (fill_value(op, T)[0],)) for op, bad, good, _ in C.fail_unary(T)]
    plant_loss(gpu_ctx, T, mode, lambda op, f: C.U(op, C.feat(f)), fu, 1, tails)
    fb = [(op, (bx, by), (gx, gy), (gx, gy)) for op, bx, by, gx, gy, _ in C.fail_binary(T)]
    plant_loss(gpu_ctx, T, mode, lambda op, f: C.B(op, C.feat(f), C.feat(f + 1)), fb, 2, tails)
    tails.flush()


def test_planted_failures_memory_constants(gpu_ctx):
    """The binary failure entries whose bad and good pairs share an operand, with that operand as the constant
    (c ∘ x or x ∘ c) of memory-constant code; the entries that share none (listed) cannot be planted this way."""
    T = np.float32
    tails = Tails("planted failures, memory-constant code", T)
    fb = C.fail_binary(T)
    left = [e for e in fb if e[1] == e[3] and np.signbit(e[1]) == np.signbit(e[3])]
    right = [e for e in fb if e not in left and e[2] == e[4] and np.signbit(e[2]) == np.signbit(e[4])]
    neither = [(e[0], e[1], e[2]) for e in fb if e not in left and e not in right]
    assert [e[0] for e in neither] == ["*"] and neither[0][1] == neither[0][2] == float(np.float32(1e20)), neither
    assert len(left) >= 20 and len(right) >= 1, (len(left), len(right))
    for side, ents in (("left", left), ("right", right)):
        for e0 in range(0, len(ents), 4):
            part = ents[e0:e0 + 4]
            names, inner = [], []
            X = np.empty((2 * len(part), NROWS))
            Xg = np.empty_like(X)
            rows = []
            for i, (op, bx, by, gx, gy, _) in enumerate(part):
                c, bad, good = (bx, by, gy) if side == "left" else (by, bx, gx)
                r = PLANT_ROWS[(e0 + i + 2) % len(PLANT_ROWS)]
                rows.append(r)
                for tree, val in ((0, bad), (1, good)):
                    f = 2 * i + tree
                    X[f], Xg[f] = good, good
                    X[f, r] = val
                    k = srhip.Node(val=float(np.float32(c)))
                    inner.append(C.B(op, k, C.feat(f + 1)) if side == "left" else C.B(op, C.feat(f + 1), k))
                    names.append(op)
            batch = LossBatch(gpu_ctx, T, "memory-constants", inner, names, 2 * len(part))
            out = batch.outputs(Xg)
            xj = out.astype(np.float64)
            for i, r in enumerate(rows):
                xj[2 * i, r] = 0.0
            s, ok = batch.sums(X, xj)
            assert list(ok) == [False, True] * len(part), (side, [(e[:5], bool(ok[2 * i]), bool(ok[2 * i + 1])) for i, e in enumerate(part)])
            for i, e in enumerate(part):
                assert np.isnan(s[2 * i]) and s[2 * i + 1] == 0.0, (e, s[2 * i], s[2 * i + 1])
                tails.add(e[0], 0.0)
    tails.flush()


# ---- j. the gradient tree code's own rules ----------------------------------------------------------
# jit_grad.cpp / jit64.cpp compile `+ - * / ^` and neg abs square cube exp sin cos log sqrt with derivative rules
# of their own. eval_loss_grad with L2 under SRHIP_GJIT=1 on the grids of tests/golden/derivatives.npz, against
# Σ 2 r · (fixture derivative): test_derivative_rules_gpu.l2_reference and its bound, unchanged.

GRAD_UNARY = ("neg", "abs", "square", "cube", "exp", "sin", "cos", "log", "sqrt")
GRAD_BINARY = ("+", "-", "*", "/", "pow")
GRAD_SAFE = {"log": -2.0, "sqrt": -2.0, "pow": -2.0, "/": 0.0}  # an out-of-domain operand per safe operator


def grad_problem(T):
    """(names, trees, X, per tree [(true ∂ŷ/∂c per row, its bound)] in constant order). Unary: op(c0 + x). Binary,
    on block 0 of the operator's grid: the tangent on the left operand (op(x·c0, y)), on the right one
    (op(x, y·c0)) and on both (op(x·c0, y·c1)). Grid points with |value| and |derivative| below 1e6, as
    test_derivative_rules_gpu.slice_problem (an L2 sum of squares must stay finite in Float32)."""
    import derivative_cases as D
    from test_derivative_rules_gpu import B as DB
    from test_derivative_rules_gpu import feat as dfeat
    from test_derivative_rules_gpu import partial_tol, scaled

    nf = len(GRAD_UNARY) + 2 * len(GRAD_BINARY)
    X = np.empty((nf, NROWS))
    names, trees, terms = [], [], []
    for i, op in enumerate(GRAD_UNARY):
        x, d, sp = D.unary_case(op, T)
        with np.errstate(all="ignore"):
            v = oracle.eval_tree(*srhip.flatten([D.unary_tree(op)], D.options(), dtype=np.float64).tree(0), x[None, :], dtype=np.float64)[0]
        keep = np.flatnonzero((np.abs(v) < 1e6) & (np.abs(d) < 1e6) & np.isfinite(sp))
        r = keep[np.arange(NROWS) % len(keep)]
        X[i] = x[r]
        names.append(op), trees.append(D.unary_tree(op, i + 1))
        terms.append([(d[r], partial_tol(d[r], sp[r], D.unary_bound_ulp(op, T), T))])
    for k, op in enumerate(GRAD_BINARY):
        c = D.binary_case(op, T)
        keep = np.flatnonzero((c["block"] == 0) & (np.abs(c["x"]) < 1e3) & (np.abs(c["y"]) < 1e3) & (np.abs(c["dx"]) < 1e6)
                              & (np.abs(c["dy"]) < 1e6))
        r = keep[np.arange(NROWS) % len(keep)]
        fa, fb = len(GRAD_UNARY) + 2 * k, len(GRAD_UNARY) + 2 * k + 1
        X[fa], X[fb] = c["x"][r], c["y"][r]
        bx, by = D.binary_bound_ulp(op, T)
        tx = (c["dx"][r] * X[fa], partial_tol(c["dx"][r], c["sx"][r], bx, T, X[fa]))
        ty = (c["dy"][r] * X[fb], partial_tol(c["dy"][r], c["sy"][r], by, T, X[fb]))
        for pos, tree, tt in (("left", DB(op, scaled(fa + 1), dfeat(fb + 1)), [tx]), ("right", DB(op, dfeat(fa + 1), scaled(fb + 1)), [ty]),
                              ("both", DB(op, scaled(fa + 1), scaled(fb + 1)), [tx, ty])):
            names.append(f"{op} {pos}"), trees.append(tree), terms.append(tt)
    return names, trees, X.astype(T), terms


def grad_pow_problem(T):
    """pow's other blocks of the derivative fixture, where the tree code's rule is its own: negative bases with
    integer exponents (block 1) and base 0 (block 2), both mixed row by row with positive bases of block 0, so
    that the lanes of a wave differ in `a > 0`. ∂/∂b is the convention 0 at a <= 0 (the fixture's dy), ∂/∂a goes
    through safe_pow(a, b - 1). Positions and filter as grad_problem."""
    import derivative_cases as D
    from test_derivative_rules_gpu import B as DB
    from test_derivative_rules_gpu import feat as dfeat
    from test_derivative_rules_gpu import partial_tol, scaled

    c = D.binary_case("pow", T)
    assert sorted(np.unique(c["block"])) == [0, 1, 2] and np.all(c["x"][c["block"] == 1] < 0) and np.all(c["x"][c["block"] == 2] == 0)
    small = (np.abs(c["x"]) < 1e3) & (np.abs(c["y"]) < 1e3) & (np.abs(c["dx"]) < 1e6) & (np.abs(c["dy"]) < 1e6)
    with np.errstate(all="ignore"):
        small &= np.abs(np.where(c["x"] == 0, 0.0, np.abs(c["x"]) ** c["y"])) < 1e6
    sets = {"negative": np.flatnonzero(small & (c["block"] == 1)), "zero": np.flatnonzero(small & (c["block"] == 2)),
            "mixed": np.flatnonzero(small)}
    assert len(sets["negative"]) >= 25 and len(sets["zero"]) >= 3
    X = np.empty((2 * len(sets), NROWS))
    names, trees, terms = [], [], []
    bx, by = D.binary_bound_ulp("pow", T)
    for k, (what, keep) in enumerate(sets.items()):
        r = keep[np.arange(NROWS) % len(keep)]
        fa, fb = 2 * k, 2 * k + 1
        X[fa], X[fb] = c["x"][r], c["y"][r]
        tx = (c["dx"][r] * X[fa], partial_tol(c["dx"][r], c["sx"][r], bx, T, X[fa]))
        ty = (c["dy"][r] * X[fb], partial_tol(c["dy"][r], c["sy"][r], by, T, X[fb]))
        for pos, tree, tt in (("left", DB("pow", scaled(fa + 1), dfeat(fb + 1)), [tx]), ("right", DB("pow", dfeat(fa + 1), scaled(fb + 1)), [ty]),
                              ("both", DB("pow", scaled(fa + 1), scaled(fb + 1)), [tx, ty])):
            names.append(f"pow {what} {pos}"), trees.append(tree), terms.append(tt)
    return names, trees, X.astype(T), terms


def grad_run(ctx, flat, T, ds, gjit):
    """eval_loss_grad of a fresh program with the gradient tree code on or off; asserts which one ran."""
    with env(SRHIP_GJIT="1" if gjit else "0"):
        prog = srhip.Program(ctx, flat, T)
        s, g, wsum, ok = prog.eval_loss_grad(ds, L2.kind, L2.params)
        name, ran, info = ctx.last_kernel_name(), ctx.last_tree_code(), prog.grad_jit_info()
    if gjit:
        assert info["ntrees"] == flat.ntrees and info["nrejected"] == 0 and ran == flat.ntrees, (info, ran)
        assert name == ("sr_jit_grad_dl" if np.dtype(T) == np.float32 else "sr_jit64_grad_dl"), name
    else:
        assert info["ntrees"] == 0 and ran == 0 and name == f"grad_kernel<{CNAME[np.dtype(T)]}>", (info, ran, name)
    return np.array(s, copy=True), np.array(g, copy=True), np.array(ok, copy=True)


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
@pytest.mark.parametrize("problem", [grad_problem, grad_pow_problem], ids=["all-operators", "pow-bases-below-and-at-0"])
def test_gradient_tree_code_rules(gpu_ctx, problem, T):
    from test_derivative_rules_gpu import check_l2, l2_reference

    ctx = gpu_ctx
    names, trees, XT, terms = problem(T)
    flat = srhip.flatten(trees, C.options(), dtype=T)
    nc = [len(t) for t in terms]
    assert list(np.diff(flat.const_off)) == nc
    y = np.random.default_rng(5).uniform(-1, 1, NROWS).astype(T)
    ds = srhip.DeviceDataset(ctx, XT, y)
    off = np.concatenate([[0], np.cumsum(nc)])
    zero = np.zeros(NROWS)
    for gjit in (True, False):
        s, g, ok = grad_run(ctx, flat, T, ds, gjit)
        assert ok.all(), [n for n, k in zip(names, ok) if not k]
        tails = Tails("gradient tree code" if gjit else "gradient interpreter (same trees)", T)
        for j in (0, 1):  # the j-th constant of every tree that has one
            sel = [t for t in range(len(trees)) if nc[t] > j]
            true = [terms[t][j][0] if nc[t] > j else zero for t in range(len(trees))]
            tol = [terms[t][j][1] if nc[t] > j else zero for t in range(len(trees))]
            ref, bound = l2_reference(flat, XT, y, true, tol, T)
            check_l2(g[off[sel] + j], ref[sel], bound[sel], [f"{names[t]} c{j}" for t in sel], tails, "gjit" if gjit else "interp")
        tails.flush()


@pytest.mark.parametrize("T", C.DTYPES, **TIDS)
def test_gradient_tree_code_out_of_domain_row(gpu_ctx, T):
    """One out-of-domain row per safe operator the gradient tree code compiles: the tree fails, its sum and every
    one of its constants' gradients are NaN; a healthy tree of the same batch keeps its gradient."""
    import derivative_cases as D
    from test_derivative_rules_gpu import B as DB

    ctx = gpu_ctx
    names = list(GRAD_SAFE)
    X = np.random.default_rng(9).uniform(1.5, 3.0, (len(names) + 1, NROWS))
    trees = []
    for i, op in enumerate(names):
        X[i, PLANT_ROWS[(i + 4) % len(PLANT_ROWS)]] = GRAD_SAFE[op]
        if op == "pow":
            trees.append(DB("pow", D.carrier(i + 1), srhip.Node(val=0.5)))
        elif op == "/":
            trees.append(DB("/", srhip.Node(val=1.5), D.carrier(i + 1)))
        else:
            trees.append(DB("*", srhip.Node(val=1.5), D.unary_tree(op, i + 1)))
    trees.append(DB("*", srhip.Node(val=1.5), D.unary_tree("square", len(names) + 1)))
    flat = srhip.flatten(trees, C.options(), dtype=T)
    assert list(np.diff(flat.const_off)) == [2] * len(trees)
    ds = srhip.DeviceDataset(ctx, X.astype(T), np.zeros(NROWS, dtype=T))
    for gjit in (True, False):
        s, g, ok = grad_run(ctx, flat, T, ds, gjit)
        assert list(ok) == [False] * len(names) + [True], ok
        assert np.isnan(s[:-1]).all() and np.isnan(g[:-2]).all() and np.isfinite(g[-2:]).all() and np.all(g[-2:] != 0), (s, g)
