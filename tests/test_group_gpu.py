"""Device groups on the GPU (include/srhip.h "device groups"): one process, the
rows sharded over the members of a group, the shards combined on the device in member order.

Every group here is made of members on device 0 ([0, 0], [0, 0, 0]): a repeated device is a
supported configuration and runs every path; where a second device is visible one case uses
[0, 1]. The yardstick of the combination is exact: the single-context API on shard datasets
(srhip_dataset_create with row_begin / row_end), combined on the host as pack_partials ->
fp64 sum left to right in shard order -> unpack_partials (srhip/distributed.py). The group's
results must equal that bit for bit. Against the oracle on the whole dataset the bars are the
project's own (tests/numerics.py, as tests/test_wide_gpu.py uses them).
"""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the engine opens the device: the process then holds one HIP runtime)

import expr_loss_cases as EL
import oracle
import srhip
from numerics import assert_close_conditioned, loss_spread
from srhip import Node
from srhip._lib import ERR_INVALID
from srhip.constant_optimization import _finish, _grad_finish, start_noise
from srhip.distributed import (pack_grad_partials, pack_partials, shard_range, unpack_grad_partials,
                               unpack_partials)
from test_gradients import grad_spread

pytestmark = pytest.mark.gpu

DTYPES = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
OPS = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
L2 = srhip.L2DistLoss()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same_bits(a, b):
    """Equal bit patterns, NaN positions equal (the payload of a NaN is not compared)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a[~na]), bits(b[~nb]))


@functools.lru_cache(maxsize=None)
def problem(T, n=1000, ntrees=40, classes=False):
    """(options, trees, flat, X, y, w): random trees over {+, -, *, /, cos, exp}, 5 features."""
    T = np.dtype(T).type
    o = srhip.Options(**OPS)
    trees = list(srhip.random_population(ntrees, o, 5, T, seed=11))
    flat = srhip.flatten(trees, o, dtype=T)
    X = np.random.default_rng(12).standard_normal((5, n)).astype(T)
    y = (T(2) * np.cos(X[3]) + X[0] * X[0] - T(2)).astype(T)
    if classes:
        y = np.where(y >= 0, 1, -1).astype(T)
    w = np.abs(np.random.default_rng(13).standard_normal(n)).astype(T)
    for a in (X, y, w):
        a.setflags(write=False)
    return o, trees, flat, X, y, w


def shard_datasets(ctx, X, y, w, ndev):
    n = X.shape[1]
    return [srhip.DeviceDataset(ctx, X, y, w, *shard_range(n, k, ndev)) for k in range(ndev)]


def host_combined_loss(ctx, flat, T, X, y, w, ndev, loss):
    """The reference of the combination: eval_loss per shard with ONE single-context program,
    packed, added left to right in shard order, unpacked. Each shard is evaluated twice and
    must repeat itself, so that a mismatch of the group points at the group."""
    prog = srhip.Program(ctx, flat, T)
    total = None
    for ds in shard_datasets(ctx, X, y, w, ndev):
        s, ws, ok = prog.eval_loss(ds, loss.kind, loss.params)
        s2, ws2, ok2 = prog.eval_loss(ds, loss.kind, loss.params)
        assert same_bits(s, s2) and ws == ws2 and np.array_equal(ok, ok2), "the single-context call does not repeat"
        part = pack_partials(s, ws, ok)
        total = part if total is None else total + part
    return unpack_partials(total)


def check_group_loss(ctx, devices, flat, T, X, y, w, loss, what):
    ref_s, ref_w, ref_ok = host_combined_loss(ctx, flat, T, X, y, w, len(devices), loss)
    with srhip.DeviceGroup(devices) as g:
        gds = g.dataset(X, y, w)
        prog = g.program(flat, T)
        s, ws, ok = prog.eval_loss(gds, loss.kind, loss.params)
        tree_code = [g.context(k).last_tree_code() for k in range(g.ndev)]
    assert np.array_equal(ok, ref_ok), (what, np.flatnonzero(ok != ref_ok))
    assert same_bits(s, ref_s), (what, np.flatnonzero(bits(s) != bits(ref_s)))
    assert same_bits([ws], [ref_w]), (what, ws, ref_w)
    return s, ws, ok, tree_code


def check_against_oracle(s, ws, ok, trees, o, flat, T, X, y, w, what, min_compared):
    with np.errstate(all="ignore"):
        losses = (s / ws).astype(T)
        losses[~ok] = T(np.inf)
        _, ref, rok = oracle.eval_loss_batch(flat, X, y, w, dtype=T)
        wsum = float(X.shape[1]) if w is None else float(w.astype(np.float64).sum())
        spread = loss_spread(trees, o, X, y, w, T) / wsum
    assert np.array_equal(ok, rok), (what, np.flatnonzero(ok != rok))
    m = ok & np.isfinite(ref)
    print(f"{what}: {int(m.sum())} trees compared with the oracle")
    assert m.sum() >= min_compared, (what, int(m.sum()))
    assert_close_conditioned(losses[m], ref[m], spread[m], rtol=1e-5 if T == np.float32 else 1e-9, msg=what)


# ---- 1. bit for bit against the shards, 2. against the oracle --------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("T", DTYPES)
def test_interpreter_batch_l2(gpu_ctx, T, weighted):
    """40 trees (interpreter: below the 256-tree bar of the tree code), 1000 rows over three
    members (334 / 333 / 333). Of the 40 trees the oracle scores 33 (Float32) / 36 (Float64)
    with a finite loss on these rows."""
    o, trees, flat, X, y, w = problem(T)
    wv = w if weighted else None
    assert [shard_range(1000, k, 3) for k in range(3)] == [(0, 334), (334, 667), (667, 1000)]
    what = f"L2 {np.dtype(T).name} weighted={weighted}"
    s, ws, ok, tc = check_group_loss(gpu_ctx, [0, 0, 0], flat, T, X, y, wv, L2, what)
    assert tc == [0, 0, 0], tc
    check_against_oracle(s, ws, ok, trees, o, flat, T, X, y, wv, what, 30)


@pytest.mark.parametrize("loss_name", ["huber", "l1hinge", "expr"])
def test_interpreter_batch_other_losses(gpu_ctx, loss_name):
    """The generic loss tail (Huber), a margin loss on y in {-1, +1}, and the expression loss
    E2 of tests/expr_loss_cases.py; Float32, unweighted, three members."""
    T = np.float32
    loss = {"huber": lambda: srhip.HuberLoss(0.8), "l1hinge": srhip.L1HingeLoss,
            "expr": lambda: EL.expr_loss("E2")}[loss_name]()
    o, trees, flat, X, y, w = problem(T, classes=loss_name == "l1hinge")
    s, ws, ok, tc = check_group_loss(gpu_ctx, [0, 0, 0], flat, T, X, y, None, loss, loss_name)
    assert ok.sum() >= 30 and not ok.all()


def test_empty_shard(gpu_ctx):
    """One tree, two rows, three members: the last shard is empty and launches nothing."""
    T = np.float32
    o = srhip.Options(**OPS)
    trees = [o.make_binary("+", o.make_unary("cos", Node(feature=1)), Node(val=0.5))]
    flat = srhip.flatten(trees, o, dtype=T)
    X = np.array([[0.25, -1.5], [1.0, 2.0]], dtype=T)
    y = np.array([1.0, 0.5], dtype=T)
    assert shard_range(2, 2, 3) == (2, 2)
    s, ws, ok, tc = check_group_loss(gpu_ctx, [0, 0, 0], flat, T, X, y, None, L2, "empty shard")
    assert ok.all() and ws == 2.0
    want = np.sum((np.cos(X[0].astype(np.float64)) + 0.5 - y) ** 2)
    np.testing.assert_allclose(s[0], want, rtol=1e-5)


def test_tree_code(gpu_ctx):
    """300 trees (above the 256-tree bar), 16500 rows over two members: 8250 rows each, more
    than one 8192-row block per shard with a padded tail. Both members ran tree code. The
    oracle scores 238 of the 300 trees with a finite loss."""
    T = np.float32
    o, trees, flat, X, y, w = problem(T, n=16500, ntrees=300)
    assert [shard_range(16500, k, 2) for k in range(2)] == [(0, 8250), (8250, 16500)]
    s, ws, ok, tc = check_group_loss(gpu_ctx, [0, 0], flat, T, X, y, None, L2, "tree code")
    assert all(n > 0 for n in tc), tc
    check_against_oracle(s, ws, ok, trees, o, flat, T, X, y, None, "tree code", 200)


def test_two_devices(gpu_ctx):
    """The interpreter batch on [0, 1] where a second device is visible."""
    if srhip.device_count() < 2:
        pytest.skip("one device visible")
    T = np.float32
    o, trees, flat, X, y, w = problem(T)
    s, ws, ok, tc = check_group_loss(gpu_ctx, [0, 1], flat, T, X, y, w, L2, "[0, 1]")
    check_against_oracle(s, ws, ok, trees, o, flat, T, X, y, w, "[0, 1]", 30)


# ---- 3. failure on one shard only -----------------------------------------------------------
@pytest.mark.parametrize("row", [900, 5], ids=["last-shard", "first-shard"])
def test_failure_on_one_shard(gpu_ctx, row):
    """x1 = 1000 in one row: exp(x1) overflows there, so exp(x1) and exp(x1)*0 + x2 fail on
    that shard alone and must fail for the group; x2 succeeds. As the oracle says on the
    whole dataset."""
    T = np.float32
    o = srhip.Options(**OPS)
    B, U = o.make_binary, o.make_unary
    trees = [U("exp", Node(feature=1)), B("+", B("*", U("exp", Node(feature=1)), Node(val=0.0)), Node(feature=2)),
             Node(feature=2)]
    flat = srhip.flatten(trees, o, dtype=T)
    X = np.array(problem(T)[3][:2])
    X[0, row] = T(1000.0)
    y = np.array(problem(T)[4])
    with srhip.DeviceGroup([0, 0, 0]) as g:
        s, ws, ok = g.program(flat, T).eval_loss(g.dataset(X, y), L2.kind, L2.params)
    with np.errstate(all="ignore"):
        _, ref, rok = oracle.eval_loss_batch(flat, X, y, dtype=T)
    assert list(ok) == [False, False, True] and np.array_equal(ok, rok)
    assert np.isnan(s[0]) and np.isnan(s[1]) and np.isfinite(s[2])
    np.testing.assert_allclose(np.float32(s[2] / ws), ref[2], rtol=1e-5)


# ---- 4. gradients ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_problem(T):
    """30 trees with constants over features 1..5 of a 6-feature dataset, and exp(c * x6):
    x6 = 1000 in row 900 (the third shard of three), so that tree fails on that shard alone."""
    T = np.dtype(T).type
    o = srhip.Options(**OPS)
    pop = srhip.random_population(200, o, 5, T, seed=11)
    trees = [t for t in pop if srhip.has_constants(t)][:29]
    trees.append(o.make_unary("exp", o.make_binary("*", Node(val=1.0), Node(feature=6))))
    assert len(trees) == 30
    X = np.array(np.random.default_rng(12).standard_normal((6, 1000)).astype(T))
    X[5, 900] = T(1000.0)
    y = (T(2) * np.cos(X[3]) + X[0] * X[0] - T(2)).astype(T)
    X.setflags(write=False)
    y.setflags(write=False)
    return o, trees, srhip.flatten(trees, o, dtype=T), X, y


@pytest.mark.parametrize("loss_name", ["L2", "Huber"])
@pytest.mark.parametrize("T", DTYPES)
def test_gradients_equal_the_host_combination(gpu_ctx, T, loss_name):
    loss = L2 if loss_name == "L2" else srhip.HuberLoss(0.8)
    o, trees, flat, X, y = grad_problem(T)
    co = np.asarray(flat.const_off)
    prog = srhip.Program(gpu_ctx, flat, T)
    total, shard_ok = None, []
    for ds in shard_datasets(gpu_ctx, X, y, None, 3):
        s, g, ws, ok = prog.eval_loss_grad(ds, loss.kind, loss.params)
        shard_ok.append(ok)
        part = pack_grad_partials(s, g, ws, ok, co)
        with np.errstate(invalid="ignore"):  # infinite partials of opposite sign add to NaN, as on the device
            total = part if total is None else total + part
    ref_s, ref_g, ref_w, ref_ok = unpack_grad_partials(total, flat.ntrees, co)
    assert shard_ok[0][-1] and shard_ok[1][-1] and not shard_ok[2][-1]  # exp(c*x6) fails on the third shard only
    with srhip.DeviceGroup([0, 0, 0]) as grp:
        s, g, ws, ok = grp.program(flat, T).eval_loss_grad(grp.dataset(X, y), loss.kind, loss.params)
    assert np.array_equal(ok, ref_ok)
    assert same_bits(s, ref_s) and same_bits(g, ref_g) and same_bits([ws], [ref_w])
    assert not ok[-1] and np.isnan(s[-1]) and np.all(np.isnan(g[co[-2]:co[-1]]))
    assert ok.sum() >= 20  # the other trees' constants are untouched: equal to the reference above


def test_periodic_gradients_with_gradient_tree_code(gpu_ctx):
    """Float32 Periodic above the 256-tree bar of the gradient tree code: a member re-evaluates
    the trees its tree code failed through the host and packs its finished
    results into its slot itself. 300 trees with constants, 1000 rows, two members; equal to the
    host combination bit for bit, and gradient tree code ran on both members. The oracle
    evaluates 253 of the 300 trees successfully on these rows."""
    T = np.float32
    loss = srhip.PeriodicLoss(1.5)
    o = srhip.Options(**OPS)
    pop = srhip.random_population(700, o, 5, T, seed=11)
    trees = [t for t in pop if srhip.has_constants(t)][:300]
    assert len(trees) == 300
    flat = srhip.flatten(trees, o, dtype=T)
    co = np.asarray(flat.const_off)
    _, _, _, X, y, _ = problem(T)
    prog = srhip.Program(gpu_ctx, flat, T)
    total = None
    for ds in shard_datasets(gpu_ctx, X, y, None, 2):
        s, g, ws, ok = prog.eval_loss_grad(ds, loss.kind, loss.params)
        part = pack_grad_partials(s, g, ws, ok, co)
        with np.errstate(invalid="ignore"):
            total = part if total is None else total + part
    assert prog.grad_jit_info()["ntrees"] > 0
    ref_s, ref_g, ref_w, ref_ok = unpack_grad_partials(total, flat.ntrees, co)
    with srhip.DeviceGroup([0, 0]) as grp:
        s, g, ws, ok = grp.program(flat, T).eval_loss_grad(grp.dataset(X, y), loss.kind, loss.params)
        tc = [grp.context(k).last_tree_code() for k in range(2)]
    assert all(n > 0 for n in tc), tc
    assert np.array_equal(ok, ref_ok) and ok.sum() >= 150
    assert same_bits(s, ref_s) and same_bits(g, ref_g) and same_bits([ws], [ref_w])


@pytest.mark.parametrize("T", DTYPES)
def test_gradients_match_the_oracle(gpu_ctx, T):
    """srhip.eval_loss_grad_batch on a GroupDataset (L2) against the oracle's forward mode with
    the bar of tests/test_wide_gpu.py test_loss_gradients_match_the_oracle: per constant
    rtol * mean_i|2 r_i dy_i/dc| (1e-5 Float32, 1e-9 Float64) + 4 x the conditioned spread.
    On the CPU the oracle leaves 107 (Float32) / 117 (Float64) of the 123 constants to check."""
    o, trees, flat, X, y = grad_problem(T)
    with srhip.DeviceGroup([0, 0, 0]) as grp:
        gds = grp.dataset(X, y)
        losses, grads, ok = srhip.eval_loss_grad_batch(trees, gds, o)
        ref_l, ref_ok = srhip.eval_loss_batch_ok(trees, gds, o)
    with np.errstate(all="ignore"):
        _, ok_T = oracle.eval_trees(flat, X, dtype=T)
    assert np.array_equal(ok, ok_T) and np.array_equal(ok, ref_ok)
    rtol = 1e-5 if T == np.float32 else 1e-9
    got, ref, spread, mag = [], [], [], []
    y64 = y.astype(np.float64)
    for t, tree in enumerate(trees):
        with np.errstate(all="ignore"):
            v0, g0, rok, sv, sg = grad_spread(tree, o, X, T)
            if not (ok[t] and rok):
                continue
            r = v0 - y64
            got.append(np.asarray(grads[t], dtype=np.float64))
            ref.append(np.mean(2 * r * g0, axis=1))
            mag.append(np.mean(np.abs(2 * r * g0), axis=1))
            spread.append(np.mean(2 * (np.abs(r) * sg + np.abs(g0) * sv + sv * sg), axis=1))
    cat = np.concatenate
    got, ref, spread, mag = cat(got), cat(ref), cat(spread), cat(mag)
    fin = np.isfinite(ref) & np.isfinite(mag) & (len(y) * mag < float(np.finfo(T).max) * 2.0 ** -10)
    print(f"group loss gradients {np.dtype(T).name}: {int(fin.sum())} constants checked")
    assert fin.sum() >= 100
    assert_close_conditioned(got[fin], ref[fin], spread[fin] + rtol * mag[fin] / 4, rtol=0.0, msg="dL/dc")
    m = ok & np.isfinite(ref_l)
    np.testing.assert_allclose(losses[m], ref_l[m], rtol=rtol)


# ---- 5. set_constants -----------------------------------------------------------------------
@pytest.mark.parametrize("T", DTYPES)
def test_set_constants(gpu_ctx, T):
    o, trees, flat, X, y = grad_problem(T)
    new = (np.asarray(flat.consts, dtype=np.float64) * 1.25 + 0.125).astype(T)
    fresh = srhip.node.FlatTrees(flat.node_off, flat.kind, flat.arg, flat.const_off, new, flat.nodes)
    with srhip.DeviceGroup([0, 0]) as g:
        gds = g.dataset(X, y)
        prog = g.program(flat, T)
        before = prog.eval_loss(gds, L2.kind)
        prog.set_constants(new)
        after = prog.eval_loss(gds, L2.kind)
        want = g.program(fresh, T).eval_loss(gds, L2.kind)
        with pytest.raises(ValueError):
            prog.set_constants(new[:-1])
    assert same_bits(after[0], want[0]) and np.array_equal(after[2], want[2]) and after[1] == want[1]
    assert not same_bits(after[0], before[0])


# ---- 6. constant optimisation ---------------------------------------------------------------
class HostShardEvaluator:
    """RowShardedEvaluator's construction with a local sum in place of the all-reduce: one
    single-context program of the candidates, evaluated per shard, the partials added on the
    host in shard order."""

    def __init__(self, ctx, cands, o, T, shards):
        self.T, self.o, self.shards = T, o, shards
        self.flat = srhip.flatten(cands, o, dtype=T)
        self.co = np.asarray(self.flat.const_off)
        self.prog = srhip.Program(ctx, self.flat, T, varying_constants=True)
        self.loss = o.elementwise_loss

    def loss_grad(self, consts):
        self.prog.set_constants(np.asarray(consts).astype(self.T))
        total = None
        for ds in self.shards:
            s, g, ws, ok = self.prog.eval_loss_grad(ds, self.loss.kind, self.loss.params)
            part = pack_grad_partials(s, g, ws, ok, self.co)
            total = part if total is None else total + part
        s, g, W, k = unpack_grad_partials(total, self.flat.ntrees, self.co)
        return _finish(s, W, k), _grad_finish(g, W, k, self.co)

    def loss_only(self, consts):
        self.prog.set_constants(np.asarray(consts).astype(self.T))
        total = None
        for ds in self.shards:
            s, ws, ok = self.prog.eval_loss(ds, self.loss.kind, self.loss.params)
            part = pack_partials(s, ws, ok)
            total = part if total is None else total + part
        s, W, k = unpack_partials(total)
        return _finish(s, W, k)


@pytest.mark.parametrize("algorithm", ["BFGS", "NelderMead"])
@pytest.mark.parametrize("T", DTYPES)
def test_constant_optimisation(gpu_ctx, T, algorithm):
    """20 trees, 700 rows, two members, fixed start noise: srhip_group_optimize_constants
    returns what srhip_optimize_constants_cb returns over the host combination of the shards,
    bit for bit. srhip_group_optimize_constants gives its losses in T, as
    srhip_optimize_constants_batch does (srhip.h), and the callback entry in double: the
    callback's losses are rounded to T before they are compared. The returned losses are no
    worse than the start losses (the bar of tests/test_wide_gpu.py test_constant_optimisation)."""
    T = np.dtype(T).type
    o = srhip.Options(optimizer_algorithm=algorithm, **OPS)
    pop = srhip.random_population(200, o, 5, T, seed=11)
    base = [t for t in pop if srhip.has_constants(t)][:20]
    X = np.random.default_rng(12).standard_normal((5, 700)).astype(T)
    y = (T(2) * np.cos(X[3]) + X[0] * X[0] - T(2)).astype(T)
    noise = start_noise(srhip.flatten(base, o, dtype=T), 2, np.random.default_rng(52))
    a, b = [t.copy() for t in base], [t.copy() for t in base]
    shards = shard_datasets(gpu_ctx, X, y, None, 2)
    ref = srhip.optimize_constants_batch(srhip.Dataset(X, y), b, o, noise=noise,
                                         evaluator_factory=lambda c: HostShardEvaluator(gpu_ctx, c, o, T, shards))
    with srhip.DeviceGroup([0, 0]) as g:
        gds = g.dataset(X, y)
        start, ok0 = srhip.eval_loss_batch_ok(base, gds, o)
        res = srhip.optimize_constants_batch(gds, a, o, noise=noise)
    assert np.array_equal(res.converged, ref.converged)
    assert same_bits(res.num_evals, ref.num_evals)
    assert same_bits(res.losses, ref.losses.astype(T).astype(np.float64))
    ca = np.asarray(srhip.flatten(a, o, dtype=T).consts, dtype=np.float64)
    cb = np.asarray(srhip.flatten(b, o, dtype=T).consts, dtype=np.float64)
    assert same_bits(ca, cb)
    got = np.asarray(res.losses).astype(T)
    print(f"{algorithm} {np.dtype(T).name}: converged {int(res.converged.sum())} of 20")
    assert np.all(got[ok0] <= start[ok0]), (got, start)
    if algorithm == "BFGS":  # (8 Nelder-Mead iterations meet Optim's convergence test for no tree here,
        # with the callback evaluator as with the group: every tree then keeps x0)
        assert res.converged.any() and np.any(got[ok0] < start[ok0])


# ---- 7. lifetime ----------------------------------------------------------------------------
def test_lifetime(gpu_ctx):
    T = np.float32
    o, trees, flat, X, y, w = problem(T)
    g = srhip.DeviceGroup([0, 0])
    gds, prog = g.dataset(X, y, w), g.program(flat, T)
    alone = prog.eval_loss(gds, L2.kind)
    # two groups alive at once give what one after the other gives
    h = srhip.DeviceGroup([0, 0])
    hds, hprog = h.dataset(X, y, w), h.program(flat, T)
    r1, r2 = hprog.eval_loss(hds, L2.kind), prog.eval_loss(gds, L2.kind)
    for r in (r1, r2):
        assert same_bits(r[0], alone[0]) and np.array_equal(r[2], alone[2]) and r[1] == alone[1]
    # a program of another group
    with pytest.raises(srhip.SrhipError) as e:
        hprog.eval_loss(gds, L2.kind)
    assert e.value.code == ERR_INVALID
    assert g.info() == (0, 0) and g.context(1).device == 0
    gds.close()
    prog.close()
    g.close()
    h.close()
    with pytest.raises(ValueError):
        g.program(flat, T)
    # device 0 is still usable
    losses, ok = srhip.eval_loss_batch_ok(trees, srhip.Dataset(X, y, w), o)
    check_against_oracle(losses.astype(np.float64), 1.0, ok, trees, o, flat, T, X, y, w, "after the groups", 30)
