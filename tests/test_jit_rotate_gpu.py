"""The loss tree code's rotated tree walk and its trimmed tile (csrc/jit.cpp
launch and Gen, csrc/jit_template.hip rot_of).

Each row group starts its walk over a tree group's list at an offset of its
own (SRHIP_JIT_ROTATE: 0 off, 1 the row groups resident together at the start,
2 every row group), so list position i = (k + rot) mod tpb for claim k. The
tile's trimmed root mark has a build-time knob (TRIMS below). Neither may
change a bit of a result:

  * loss sums and did_succeed are bit-identical between SRHIP_JIT_ROTATE=0, 1
    and 2 in every loop that walks the list (the prefetching hand-written loop,
    the plain one, the memory-constant one and the compiled fallback), and
    between the trim on and off (FAST, PRECISE only, memory-constant code);
  * did_succeed equals the oracle's on every tree, and the losses of the
    succeeding trees are within 1e-5 (relative) of the oracle's (a sum beyond
    Float32's range is infinite in the engine's Float32 partial sums).

Shapes: 257 and 300 trees (just above the 256-tree bar for tree code, no
multiple of the tree-group count) on 5000 rows: five row groups of 1024 rows,
the last with a partial tile, four list positions per tree group (the
geometry's minimum, csrc/kernels.hip plan_geometry), so every row group but
the first and the fifth wraps, and the 257-tree list leaves the last position
of three tree groups empty, which a rotated walk meets before its end. 300
trees on 1500 rows: two row groups. 900 trees on 40 000 rows: forty row
groups and longer lists. The populations are seeded random ones (about a
quarter of their trees fail on some row) plus two hand-made trees: x1 / (x0 -
x0) fails on every row, x1 / x5 on row 3333 only (x5 is zero there and is read
by no other tree), that is in one tile of one row group.

SRHIP_JIT_STICKY_TREE=0 as in tests/test_bench_outputs_gpu.py: with the mark
on, which tiles run PRECISE depends on the order in which row groups meet a
tree, which is what the rotation changes.
"""
import os

import numpy as np
import pytest

import oracle
import srhip
from srhip import constants as K

pytestmark = pytest.mark.gpu

F32 = np.float32
CFG2 = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
ONE_ROW = 3333
# build-time knobs of the trimmed tile (csrc/jit.cpp Gen): "0" keeps the earlier code
TRIMS = ["SRHIP_JIT_TRIM_ROOT"]
# the loops that walk a tree group's list (csrc/jit.cpp launch)
LOOPS = {
    "prefetching": {},
    "plain": {"SRHIP_JIT_PREFETCH": "0"},
    "memory constants": {"SRHIP_JIT_MEMC": "1"},
    "compiled": {"SRHIP_JIT_DYNLOOP": "0"},
}
KERNEL = {"prefetching": "sr_jit_eval_dlp", "plain": "sr_jit_eval_dl", "memory constants": "sr_jit_eval_dlm",
          "compiled": "sr_jit_eval"}
SHAPES = [(257, 5000), (300, 5000), (300, 1500), (900, 40_000)]


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


def problem(ntrees, rows):
    o = srhip.Options(**CFG2)
    N = srhip.Node
    trees = srhip.random_population(ntrees - 2, o, 5, np.float32, seed=1000 + ntrees)
    every_row = o.make_binary("/", N(feature=2), o.make_binary("-", N(feature=1), N(feature=1)))
    one_row = o.make_binary("/", N(feature=2), N(feature=6))
    # in the middle of the list: neither the first nor the last tree of a walk
    trees = trees[: ntrees // 2] + [every_row, one_row] + trees[ntrees // 2:]
    rng = np.random.default_rng(ntrees + rows)
    X = rng.standard_normal((6, rows)).astype(F32)
    X[5] = rng.uniform(0.5, 2.0, rows).astype(F32)
    if rows > ONE_ROW:
        X[5, ONE_ROW] = 0
    y = (F32(2) * np.cos(X[3]) + X[0] * X[0] - F32(2)).astype(F32)
    return o, trees, X, y


_cache = {}


def reference(ntrees, rows):
    """The problem and the oracle's sums and did_succeed, computed once per shape."""
    key = (ntrees, rows)
    if key not in _cache:
        o, trees, X, y = problem(ntrees, rows)
        flat = srhip.flatten(trees, o, dtype=np.float32)
        ref_sum, _, ref_ok = oracle.eval_loss_batch(flat, X, y, dtype=np.float32)
        ref_sum.setflags(write=False)
        ref_ok.setflags(write=False)
        _cache[key] = (o, trees, X, y, flat, ref_sum, ref_ok)
    return _cache[key]


def run(flat, X, y, **kv):
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    with env(SRHIP_JIT="1", SRHIP_JIT_STICKY_TREE="0", **kv):
        prog = srhip.Program(ctx, flat, np.float32)
        sums, wsum, ok = prog.eval_loss(ds, K.LOSS["L2"])
        info = prog.jit_info()
        kernel = ctx.last_kernel_name()
    return np.array(sums, copy=True), np.array(ok, copy=True), info, kernel


def same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("loop", list(LOOPS))
@pytest.mark.parametrize("ntrees,rows", SHAPES)
def test_rotation_changes_no_bit(gpu_ctx, ntrees, rows, loop):
    o, trees, X, y, flat, ref_sum, ref_ok = reference(ntrees, rows)
    r = {mode: run(flat, X, y, SRHIP_JIT_ROTATE=mode, **LOOPS[loop]) for mode in ("0", "1", "2")}
    info = r["0"][2]
    print(f"{ntrees} trees x {rows} rows, {loop} loop: {info['ntrees']} trees of code, {info['nfast']} FAST, "
          f"{int((~r['0'][1]).sum())} failed, last kernel {r['0'][3]}")
    assert info["ntrees"] >= 0.9 * ntrees, info
    assert all(r[mode][3] == KERNEL[loop] for mode in r), [r[mode][3] for mode in r]
    for mode in ("1", "2"):
        bad = np.flatnonzero((r[mode][1] != r["0"][1]) | ~((r[mode][0] == r["0"][0]) | (np.isnan(r[mode][0]) & np.isnan(r["0"][0]))))
        assert same(r[mode], r["0"]), (mode, bad[:10])
    # the unrotated walk gives the oracle's verdicts: so does every rotated one
    assert np.array_equal(r["0"][1], ref_ok), np.flatnonzero(r["0"][1] != ref_ok)[:10]


@pytest.mark.parametrize("ntrees,rows", SHAPES)
def test_trims_change_no_bit(gpu_ctx, ntrees, rows):
    """With the FAST path and PRECISE only, and in memory-constant code."""
    o, trees, X, y, flat, ref_sum, ref_ok = reference(ntrees, rows)
    for kv in ({"SRHIP_JIT_FAST": "1"}, {"SRHIP_JIT_FAST": "0"}, {"SRHIP_JIT_MEMC": "1"}):
        ref = run(flat, X, y, **kv, **{k: "0" for k in TRIMS})
        got = run(flat, X, y, **kv)
        assert same(got, ref), kv
        assert np.array_equal(got[1], ref_ok), kv


@pytest.mark.parametrize("ntrees,rows", SHAPES)
def test_against_the_oracle(gpu_ctx, ntrees, rows):
    o, trees, X, y, flat, ref_sum, ref_ok = reference(ntrees, rows)
    sums, ok, info, _ = run(flat, X, y)  # the defaults: rotated, trimmed
    half = ntrees // 2
    assert not ref_ok[half] and (rows <= ONE_ROW or not ref_ok[half + 1])  # the hand-made trees fail
    nfail = int((~ref_ok).sum())
    assert 0.1 * ntrees < nfail < 0.4 * ntrees, nfail
    assert np.array_equal(ok, ref_ok), np.flatnonzero(ok != ref_ok)[:10]
    # The oracle adds the rows' Float32 losses in Float64; the tree code adds them in Float32 per
    # wave and row group (non-negative terms), so a sum of a succeeding tree that does not fit
    # Float32 may come out infinite (as the Float32 reference's own sum does); below that it is
    # finite and within 1e-5.
    fmax = float(np.finfo(np.float32).max) * (1 - 1e-5)
    fits = ref_ok & (ref_sum < fmax)
    over = ref_ok & ~fits
    rel = np.abs(sums[fits] - ref_sum[fits]) / np.maximum(np.abs(ref_sum[fits]), 1e-300)
    worst = np.argsort(rel)[::-1][:3]
    print(f"{ntrees} trees x {rows} rows: {nfail} fail, {int(over.sum())} sums beyond Float32, max relative loss "
          f"difference {rel.max():.3g} (trees {np.flatnonzero(fits)[worst].tolist()}: {rel[worst].tolist()})")
    assert np.all(rel <= 1e-5), np.flatnonzero(fits)[~(rel <= 1e-5)][:10]
    assert np.all(np.isinf(sums[over]) | (sums[over] >= fmax)), (np.flatnonzero(over), sums[over], ref_sum[over])
