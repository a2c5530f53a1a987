"""The tree compilers at their allocation limits, on the GPU: the ladders of
tests/tree_code_limit_cases.py run as tree code exactly up to the CPU test's literal limits (asserted
through Program.pass_info(), jit_info(), grad_jit_info() and Context.last_tree_code(), never `>=`),
the rejected rungs run in the interpreter in the same call, and every tree is checked against the
oracle with no spread allowance:

  per-row outputs   bit-identical to oracle.eval_trees in T
  loss sums         check_loss_sums of tests/test_variant_matrix_gpu.py (rtol 1e-5 Float32, 1e-9
                    Float64, times Σ w|ℓ|): L2 (the compiled tail), Huber(0.8) (a distance routine),
                    L1Hinge and LogitMargin (margin routines), weighted and not
  ∂L/∂c             check_loss_grads of the same file, every constant of every tree
  FAST / PRECISE    bit-identical sums (no transcendental: no guard can fire)

at n = 1, around the Float64 tile (128) and the Float32 tile (256), and 8192 + 257 (two row groups,
the second a lone partial tile). columns-and-pool and parts have a test of their own each. Worst err/bound per group: profiles/tree_code_limits_parity.json."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine opens the device: the process then holds one HIP runtime)

import oracle
import srhip
import tree_code_limit_cases as L
from test_variant_matrix_gpu import MARGIN_KINDS, Worst, check_loss_grads, check_loss_sums, dataset, env, lname

pytestmark = pytest.mark.gpu

LOSSES = [srhip.L2DistLoss(), srhip.HuberLoss(0.8), srhip.L1HingeLoss(), srhip.LogitMarginLoss()]
ON = dict(SRHIP_JIT="1", SRHIP_GJIT="1")  # tree code whatever the batch size
# (a program flagged for wide code takes it when a candidate reads a feature from index 63 on: the
# wide-window family and two ladders of high-features; elsewhere it is the LDS code of loss32)

# the program of a compiler: (keywords of srhip.Program, extra switches)
PROGRAMS = {
    "loss32": (dict(), dict()),
    "loss32p": (dict(), dict(SRHIP_JIT_FAST="0")),
    "memc32": (dict(varying_constants=True), dict()),
    "wide32": (dict(wide_tree_code=True), dict()),
    "loss64": (dict(), dict()),
    "grad32": (dict(), dict()),
    "grad64": (dict(), dict()),
}
GENERIC = [f for f in L.FAMILIES if f != "columns-and-pool"]  # (that family: test_columns_and_pool)
LOSS_CELLS = [pytest.param(f, c, id=f"{f}-{c}") for f in GENERIC for c in L.APPLIES[f]
              if c in ("loss32", "loss32p", "memc32", "loss64") or (c == "wide32" and f in ("wide-window", "high-features"))]
OUT_CELLS = [pytest.param(f, c, id=f"{f}-{c}") for f in GENERIC for c in L.APPLIES[f] if c in ("out32", "out64")]
GRAD_CELLS = [pytest.param(f, c, id=f"{f}-{c}") for f in GENERIC for c in L.APPLIES[f] if c in L.GRAD]


def runs_wide(lad, weighted, grad):
    """A loss call of an unflagged program runs wholly in the wide interpreter when an interpreter
    pass of it (the rejected rungs') does not fit in LDS (api.cpp run_eval). The row tile holds y, the
    features and w: 78 features fit without weights (README: the last count that uses LDS) and not
    with them, in both dtypes; 64 features fit either way. Gradient calls and per-row outputs keep
    their tree code on all three datasets."""
    return lad == "high78" and weighted and not grad


def routed(compiler, loss, ntc, ctx=None, lad=None, weighted=False):
    """Trees a call runs as tree code, and the kernel's name checked against runs_wide. The margin
    losses have routines in the Float32 loss code only (jit.cpp has_loss_routine); the Float64 loss
    code and both gradient compilers take the losses below SRHIP_MARGIN_LOSS_BEGIN
    (has_loss_routine64, has_dloss_routine, has_dloss_routine64): a margin loss there is a call of the
    interpreter, checked like the rest."""
    if ctx is not None and compiler != "wide32":
        wide = runs_wide(lad, weighted, compiler in L.GRAD)
        assert ("wide" in ctx.last_kernel_name()) == wide, (compiler, lad, weighted, ctx.last_kernel_name())
        if wide:
            return 0
    return 0 if loss.kind in MARGIN_KINDS and compiler in ("loss64", "grad32", "grad64") else ntc


def ladders(family):
    """The high-features family has one dataset per ladder; every other family one batch."""
    return list(L.FAMILIES[family]) if family == "high-features" else [None]


def report(worst, what):
    print(worst.line(what))
    print("TREE_CODE_LIMITS_WORST " + json.dumps({"cell": what, "worst": worst.v}))


def program(ctx, flat, compiler):
    T = L.COMPILERS[compiler][0]
    return srhip.Program(ctx, flat, T, **PROGRAMS[compiler][0])


def assert_loss_routing(prog, family, compiler, ladder, nplanted=0):
    ntc = len(L.expected(family, compiler, ladder)) + nplanted
    info, jinfo = prog.pass_info(), prog.jit_info()
    assert info["tree_code"] == ntc, (family, compiler, ladder, info)
    assert jinfo["ntrees"] == ntc, (family, compiler, ladder, jinfo)
    return ntc


@pytest.mark.parametrize("family,compiler", LOSS_CELLS)
def test_loss_sums(gpu_ctx, family, compiler):
    ctx, T = gpu_ctx, L.COMPILERS[compiler][0]
    worst = Worst()
    with env(**ON, **PROGRAMS[compiler][1]):
        for lad in ladders(family):
            prog = program(ctx, L.problem(family, T, L.ROWS[0], lad).flat, compiler)
            ntc = assert_loss_routing(prog, family, compiler, lad)
            for n in L.ROWS:
                P = L.problem(family, T, n, lad)
                assert int(P.ok.sum()) == P.flat.ntrees  # the oracle's success count: every tree
                for weighted in (False, True):
                    for loss in LOSSES:
                        what = f"{family} {lad} {compiler} {lname(loss)} n={n} weighted={weighted}"
                        s, wsum, ok = prog.eval_loss(dataset(ctx, P, loss, weighted), loss.kind, loss.params)
                        assert ctx.last_tree_code() == routed(compiler, loss, ntc, ctx, lad, weighted), (what, ctx.last_tree_code(), ctx.last_kernel_name())
                        assert ctx.last_jit_events() == (0, 0), (what, ctx.last_jit_events())
                        check_loss_sums(s, ok, wsum, P, loss, weighted, worst,
                                        "margin" if loss.kind in MARGIN_KINDS else "distance", what)
    report(worst, f"{family} {compiler} loss sums")


@pytest.mark.parametrize("family,compiler", OUT_CELLS)
def test_outputs_are_the_oracles_bits(gpu_ctx, family, compiler):
    ctx, T = gpu_ctx, L.COMPILERS[compiler][0]
    uint = np.uint32 if T == np.float32 else np.uint64
    with env(**ON):
        for lad in ladders(family):
            prog = srhip.Program(ctx, L.problem(family, T, L.ROWS[0], lad).flat, T)
            ntc = len(L.expected(family, compiler, lad))
            assert prog.pass_info()["tree_code"] == ntc
            for n in L.ROWS:
                P = L.problem(family, T, n, lad)
                out, ok = prog.eval_tree_array(srhip.DeviceDataset(ctx, P.X, P.y))
                assert ctx.last_tree_code() == ntc, (family, compiler, lad, n, ctx.last_tree_code())
                assert np.array_equal(ok, P.ok) and int(P.ok.sum()) == P.flat.ntrees
                assert np.array_equal(out.view(uint), P.yhat.view(uint)), (family, lad, n, np.argwhere(out != P.yhat)[:5])


@pytest.mark.parametrize("family,compiler", GRAD_CELLS)
def test_loss_gradients(gpu_ctx, family, compiler):
    ctx, T = gpu_ctx, L.COMPILERS[compiler][0]
    worst = Worst()
    with env(**ON):
        for lad in ladders(family):
            P0 = L.problem(family, T, L.ROWS[0], lad)
            prog = srhip.Program(ctx, P0.flat, T)
            ntc = len(L.expected(family, compiler, lad))
            nconst, checked, calls = int(P0.flat.const_off[-1]), 0, 0
            for n in L.ROWS:
                P = L.problem(family, T, n, lad)
                assert int(P.ok.sum()) == P.flat.ntrees
                for weighted in (False, True):
                    for loss in LOSSES:
                        what = f"{family} {lad} {compiler} grad {lname(loss)} n={n} weighted={weighted}"
                        sg, g, wsum, okg = prog.eval_loss_grad(dataset(ctx, P, loss, weighted), loss.kind, loss.params)
                        assert ctx.last_tree_code() == routed(compiler, loss, ntc, ctx, lad, weighted), (what, ctx.last_tree_code(), ctx.last_kernel_name())
                        check_loss_sums(sg, okg, wsum, P, loss, weighted, worst, "grad-call loss", what)
                        checked += check_loss_grads(g, P, loss, weighted, worst, what)
                        calls += 1
            ginfo = prog.grad_jit_info()
            assert ginfo["ntrees"] == ntc and ginfo["nrejected"] == P0.flat.ntrees - ntc, (family, compiler, lad, ginfo)
            assert checked == calls * nconst, (checked, calls, nconst)  # no entry dropped
    report(worst, f"{family} {compiler} gradients")


@pytest.mark.parametrize("family", ["live-values", "features-held", "constants"])
def test_fast_and_precise_give_the_same_bits(gpu_ctx, family):
    ctx, T = gpu_ctx, np.float32
    res = {}
    for compiler in ("loss32", "loss32p"):
        with env(**ON, **PROGRAMS[compiler][1]):
            prog = program(ctx, L.problem(family, T, L.ROWS[0]).flat, compiler)
            assert_loss_routing(prog, family, compiler, None)
            assert prog.jit_info()["nfast"] == 0  # no transcendental: no tree has a guarded FAST path
            for n in (257, L.BIG):
                P = L.problem(family, T, n)
                for weighted in (False, True):
                    for loss in LOSSES:
                        s, wsum, ok = prog.eval_loss(dataset(ctx, P, loss, weighted), loss.kind, loss.params)
                        assert ctx.last_jit_events() == (0, 0)
                        res.setdefault((n, weighted, lname(loss)), []).append((np.array(s, copy=True), np.array(ok, copy=True)))
    for key, ((s0, ok0), (s1, ok1)) in res.items():
        assert np.array_equal(ok0, ok1) and np.array_equal(s0, s1), (family, key)


@pytest.mark.parametrize("family", ["live-values", "constants"])
def test_memory_constant_code_after_set_constants(gpu_ctx, family):
    """New constants written in place (update_stats): the results are a fresh program's at those
    constants bit for bit, and the oracle's at the new constants within the bound. The fresh program
    is a literal-constant one, an independent code path; the comparison covers the trees that are
    tree code in both (a rung that memory-constant code refuses is interpreted here and tree code
    there, and sums in another order)."""
    ctx, T = gpu_ctx, np.float32
    worst = Worst()
    with env(**ON):
        P = L.problem(family, T, L.BIG)
        flat = P.flat
        prog = program(ctx, flat, "memc32")
        ntc = assert_loss_routing(prog, family, "memc32", None)
        c64 = np.asarray(flat.consts, dtype=np.float64)
        new = (np.sign(c64) * (1.25 - np.abs(c64))).astype(T)  # still in ±[0.25, 1], every one changed but |c| = 0.625
        assert np.all((np.abs(new) >= 0.25) & (np.abs(new) <= 1)) and np.count_nonzero(new != flat.consts) >= len(new) - 1
        fresh_flat = srhip.node.FlatTrees(flat.node_off, flat.kind, flat.arg, flat.const_off, new, flat.nodes)
        fresh = program(ctx, fresh_flat, "loss32")
        assert_loss_routing(fresh, family, "loss32", None)
        both = L.expected(family, "memc32")
        assert set(both) <= set(L.expected(family, "loss32")) and len(both) == ntc
        with np.errstate(all="ignore"):
            yhat, okq = oracle.eval_trees(fresh_flat, P.X, dtype=T)
        Q = SimpleNamespace(**{**vars(P), "flat": fresh_flat, "yhat": yhat, "ok": okq})
        assert okq.all()
        for weighted in (False, True):
            for loss in LOSSES:
                ds = dataset(ctx, P, loss, weighted)
                s0, wsum, ok0 = prog.eval_loss(ds, loss.kind, loss.params)
                assert ctx.last_tree_code() == ntc
                check_loss_sums(s0, ok0, wsum, P, loss, weighted, worst, "before", f"{family} memc {lname(loss)}")
        before = prog.update_stats()
        prog.set_constants(new)
        after = prog.update_stats()
        assert after["inplace"] == before["inplace"] + 1 and after["rebuilt"] == before["rebuilt"], (before, after)
        for weighted in (False, True):
            for loss in LOSSES:
                ds = dataset(ctx, P, loss, weighted)
                s1, wsum, ok1 = prog.eval_loss(ds, loss.kind, loss.params)
                assert ctx.last_tree_code() == ntc
                s1, ok1 = np.array(s1, copy=True), np.array(ok1, copy=True)
                check_loss_sums(s1, ok1, wsum, Q, loss, weighted, worst, "after", f"{family} memc {lname(loss)} new constants")
                s2, _, ok2 = fresh.eval_loss(ds, loss.kind, loss.params)
                assert np.array_equal(ok1, ok2) and np.array_equal(s1[both], s2[both]), (family, lname(loss), weighted)
    report(worst, f"{family} memc32 before and after set_constants")


PLANTED_CELLS = [pytest.param(f, c, id=f"{f}-{c}") for f in ("live-values", "features-held")
                 for c in ("loss32", "loss64", "grad32", "grad64")] + [pytest.param("wide-window", "wide32", id="wide-window-wide32")]


@pytest.mark.parametrize("family,compiler", PLANTED_CELLS)
def test_failures_across_row_groups(gpu_ctx, family, compiler):
    """A copy of every limit rung plus x1·c, c = max(T)/2, with |x1| = 2.4 in the last valid row of the
    second row group: did_succeed as the oracle's, NaN sums and gradients for the copies, every other
    tree within its bound; the copies are tree code. Wide code redoes the tile PRECISE, which
    restarts its feature window."""
    ctx, T = gpu_ctx, L.COMPILERS[compiler][0]
    P = L.problem(family, T, L.BIG, planted=compiler)
    nplant = P.flat.ntrees - P.nfam
    assert nplant == len(L.limit_rungs(family, compiler)) > 0
    assert P.ok[:P.nfam].all() and not P.ok[P.nfam:].any()  # the oracle's success count
    worst = Worst()
    with env(**ON):
        prog = program(ctx, P.flat, compiler)
        ntc = len(L.expected(family, compiler)) + nplant
        for weighted in (False, True):
            for loss in LOSSES:
                what = f"{family} {compiler} failing batch {lname(loss)} weighted={weighted}"
                ds = dataset(ctx, P, loss, weighted)
                if compiler in L.GRAD:
                    s, g, wsum, ok = prog.eval_loss_grad(ds, loss.kind, loss.params)
                    check_loss_grads(g, P, loss, weighted, worst, what)
                else:
                    s, wsum, ok = prog.eval_loss(ds, loss.kind, loss.params)
                    if compiler == "wide32":
                        assert ctx.last_jit_events()[1] > 0, (what, ctx.last_jit_events())
                assert ctx.last_tree_code() == routed(compiler, loss, ntc), (what, ctx.last_tree_code())
                check_loss_sums(s, ok, wsum, P, loss, weighted, worst, "loss", what)
        if compiler in L.GRAD:
            assert prog.grad_jit_info()["ntrees"] == ntc
        else:
            assert_loss_routing(prog, family, compiler, None, nplant)
    report(worst, f"{family} {compiler} n={P.n}, {nplant} failing trees")


@pytest.mark.parametrize("compiler", ["loss32", "loss32p"])
def test_columns_and_pool(gpu_ctx, compiler):
    """Four shared-subtree columns x_k / x_(k+4) (Program.shared_columns()) preloaded into pool
    blocks next to F held features: the rungs up to COLS_LIMIT read their columns with a full pool,
    the rungs beyond are their own code; all of them, and the fillers, are tree code and within the
    loss bounds. (The divisions have guarded FAST paths: a redone tile is no finding here.)"""
    ctx, T, family = gpu_ctx, np.float32, "columns-and-pool"
    worst = Worst()
    with env(**ON, **PROGRAMS[compiler][1]):
        prog = program(ctx, L.problem(family, T, L.ROWS[0]).flat, compiler)
        ntc = assert_loss_routing(prog, family, compiler, None)
        assert ntc == len(L.batch(family)[0])
        cols = prog.shared_columns()
        assert len(cols) == L.NCOLS and len(set(cols.values())) == L.NCOLS, cols
        for n in L.ROWS:
            P = L.problem(family, T, n)
            assert int(P.ok.sum()) == P.flat.ntrees
            for weighted in (False, True):
                for loss in LOSSES:
                    what = f"{family} {compiler} {lname(loss)} n={n} weighted={weighted}"
                    s, wsum, ok = prog.eval_loss(dataset(ctx, P, loss, weighted), loss.kind, loss.params)
                    assert ctx.last_tree_code() == ntc, (what, ctx.last_tree_code())
                    assert ctx.last_jit_events()[0] == 0, (what, ctx.last_jit_events())  # no tree handed back
                    check_loss_sums(s, ok, wsum, P, loss, weighted, worst,
                                    "margin" if loss.kind in MARGIN_KINDS else "distance", what)
    report(worst, f"{family} {compiler} loss sums")


def test_parts(gpu_ctx):
    """Enough copies of the largest live-values rung, with distinct constants, that the code needs a
    second part (jit.cpp build): every copy is tree code, the code is larger than one area, and the
    outputs (bit for bit) and sums match the oracle on both sides of the part boundary. A second,
    small program stays within the small template's 1 MiB area, for which build lays it out again."""
    from test_tree_code_limits import parts_copies

    ctx, T = gpu_ctx, np.float32
    ncopies, per_tree = parts_copies()
    P = L.parts_problem(ncopies)
    assert int(P.ok.sum()) == ncopies
    worst = Worst()
    with env(**ON):
        prog = srhip.Program(ctx, P.flat, T)
        info = prog.jit_info()
        print(f"parts: {ncopies} trees, {info}")
        assert prog.pass_info()["tree_code"] == ncopies and info["ntrees"] == ncopies
        assert info["code_bytes"] > L.AREA_BYTES  # more than one area holds: at least two parts
        out, ok = prog.eval_tree_array(srhip.DeviceDataset(ctx, P.X, P.y))
        assert ctx.last_tree_code() == ncopies
        assert np.array_equal(ok, P.ok)
        assert np.array_equal(out.view(np.uint32), P.yhat.view(np.uint32)), np.argwhere(out != P.yhat)[:5]
        for weighted in (False, True):
            for loss in (LOSSES[0], LOSSES[2]):
                what = f"parts {lname(loss)} weighted={weighted}"
                s, wsum, ok = prog.eval_loss(dataset(ctx, P, loss, weighted), loss.kind, loss.params)
                assert ctx.last_tree_code() == ncopies and ctx.last_jit_events() == (0, 0), what
                check_loss_sums(s, ok, wsum, P, loss, weighted, worst, "loss", what)
        small = L.parts_problem(64)
        sprog = srhip.Program(ctx, small.flat, T)
        sinfo = sprog.jit_info()
        assert sinfo["ntrees"] == 64 and sinfo["code_bytes"] <= 262144 * 4 - 64, sinfo  # (csrc/Makefile: the small area)
        s, wsum, ok = sprog.eval_loss(dataset(ctx, small, LOSSES[0], False), 0, None)
        assert ctx.last_tree_code() == 64
        check_loss_sums(s, ok, wsum, small, LOSSES[0], False, worst, "small", "parts small program")
    report(worst, f"parts {ncopies} trees")
