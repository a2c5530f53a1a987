"""Wide loss tree code on the GPU (SRHIP_PROGRAM_WIDE_TREE_CODE): a flagged
Float32 program whose tree-code candidates read a feature from index 63 on runs them as tree
code that loads its features from X in device memory, on datasets whose row tile does not fit
in LDS, where an unflagged program runs wholly in the wide interpreter.

The inputs are tests/wide_cases.py's (300 random trees and 6 hand-made ones). Checked on the
CPU against the oracle, ok / compared (finite reference loss), weighted and unweighted alike:
160 x 700: 256 / 249; 300 x 700: 254 / 251; 300 x 8200: 245 / 242; 160 x 1: 303 / 303; in each
the last tree fails and the five hand-made readers of x_nfeat succeed. Bars: did_succeed equal
to the oracle's on every tree, losses within 1e-5 relative beyond the conditioned spread of
tests/numerics.py (assert_close_conditioned, as tests/test_wide_gpu.py uses it)."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the engine opens the device: the process then holds one HIP runtime)

import oracle
import srhip
import wide_cases as W
from numerics import assert_close_conditioned, loss_spread, loss_spread_flat
from srhip import constants as K
from srhip.engine import SrhipError

pytestmark = pytest.mark.gpu

F32 = np.float32
NT = 300  # random trees; 306 with the hand-made ones
L2 = 0


def run(ctx, flat, X, y, w, flagged, loss=None, row_idx=None):
    """(losses, ok, trees run as tree code, kernel name, (bailed, redone tiles), program)."""
    loss = loss or srhip.L2DistLoss()
    prog = srhip.Program(ctx, flat, F32, wide_tree_code=flagged)
    ds = srhip.DeviceDataset(ctx, X, y, w)
    s, wsum, ok = prog.eval_loss(ds, loss.kind, loss.params, row_idx)
    ntc, name, ev = ctx.last_tree_code(), ctx.last_kernel_name(), ctx.last_jit_events()
    with np.errstate(invalid="ignore", divide="ignore"):
        losses = (s / wsum).astype(F32)
    ok = np.asarray(ok).astype(bool)
    losses[~ok] = np.inf
    return losses, ok, ntc, name, ev, prog


def check_against(losses, ok, ref, rok, spread, min_compared, what):
    assert np.array_equal(ok, rok), (what, np.flatnonzero(ok != rok))
    assert not ok[-1], what  # exp(exp(exp(50·x_nfeat))) overflows
    m = ok & np.isfinite(ref)
    with np.errstate(all="ignore"):
        rel = np.abs(losses[m].astype(np.float64) - ref[m]) / np.abs(ref[m])
    print(f"{what}: {int(m.sum())} trees compared, max rel {float(np.nanmax(rel)):.3g}")
    assert m.sum() >= min_compared, (what, int(m.sum()))
    assert m[-6:-1].all(), what  # the hand-made trees reading x_nfeat are among them
    assert_close_conditioned(losses[m], ref[m], spread[m], rtol=1e-5, msg=what)
    return m


# ---- 1. parity with the oracle, and with the interpreter ------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("nfeat,n", [(160, 700), (300, 700), (300, 8200), (160, 1)])
def test_flagged_program_matches_the_oracle_and_the_interpreter(gpu_ctx, nfeat, n, weighted):
    """700 rows: three tiles, the last partial; 8200: two row groups; 1: one row of one tile.
    The unflagged program of the same trees is the no-flag check: no tree code at all."""
    what = f"wide tree code nfeat={nfeat} n={n} weighted={weighted}"
    o, trees, flat, X, y, w = W.problem(F32, nfeat, n, NT)
    wv = w if weighted else None
    ref, rok, spread = W.reference(F32, nfeat, n, NT, weighted)
    losses, ok, ntc, name, ev, _ = run(gpu_ctx, flat, X, y, wv, True)
    print(f"{what}: {ntc} trees as tree code, kernel {name}, events {ev}")
    assert ntc >= 290, (what, ntc)
    assert name == ("sr_jit_eval_dlpw" if weighted else "sr_jit_eval_dlp"), name
    m = check_against(losses, ok, ref, rok, spread, 225, what)
    assert ev[1] > 0, (what, ev)  # the failing exp(exp(exp(·))) is tree code and redoes its first tile
    # the interpreter: the same trees without the flag
    li, oki, ntci, namei, _, _ = run(gpu_ctx, flat, X, y, wv, False)
    assert ntci == 0 and "wide" in namei, (what, ntci, namei)
    assert np.array_equal(oki, ok), (what, np.flatnonzero(oki != ok))
    assert_close_conditioned(losses[m], li[m].astype(np.float64), spread[m], rtol=1e-5, msg=what + " vs interpreter")
    assert_close_conditioned(li[m], ref[m], spread[m], rtol=1e-5, msg=what + " interpreter vs oracle")


def test_flag_is_accepted_and_unknown_bits_are_invalid(gpu_ctx):
    o, trees, flat, X, y, w = W.problem(F32, 160, 700, NT)
    for kw in (dict(), dict(varying_constants=True), dict(interpreted=True)):
        srhip.Program(gpu_ctx, flat, F32, wide_tree_code=True, **kw)
    srhip.Program(gpu_ctx, flat, np.float64, wide_tree_code=True)
    import ctypes as C

    from srhip._lib import lib
    from srhip.engine import _trees_struct

    tr = _trees_struct(flat, np.ascontiguousarray(flat.consts, dtype=F32))
    h = C.c_void_p()
    for flags in (8, 4 | 8, 16):
        assert lib().srhip_program_create_ex(gpu_ctx.handle, 0, C.byref(tr), flags, C.byref(h)) == -1  # INVALID
    assert K.PROGRAM_WIDE_TREE_CODE == 4


# ---- 2. the flag's other combinations -------------------------------------------------------
def test_flag_has_no_effect_on_float64_interpreted_and_memory_constant_programs(gpu_ctx):
    o, trees, flat, X, y, w = W.problem(F32, 160, 700, NT)
    ds = srhip.DeviceDataset(gpu_ctx, X, y)
    for kw in (dict(interpreted=True), dict(varying_constants=True)):
        srhip.Program(gpu_ctx, flat, F32, wide_tree_code=True, **kw).eval_loss(ds, L2)
        assert gpu_ctx.last_tree_code() == 0 and "wide" in gpu_ctx.last_kernel_name(), kw
    o, trees, flat, X, y, w = W.problem(np.float64, 160, 700, NT)
    srhip.Program(gpu_ctx, flat, np.float64, wide_tree_code=True).eval_loss(srhip.DeviceDataset(gpu_ctx, X, y), L2)
    assert gpu_ctx.last_tree_code() == 0 and "wide" in gpu_ctx.last_kernel_name()


def test_forced_wide_interpreter_uses_no_tree_code(gpu_ctx):
    from test_wide_gpu import wide_env

    o, trees, flat, X, y, w = W.problem(F32, 160, 700, NT)
    with wide_env("1"):
        losses, ok, ntc, name, _, _ = run(gpu_ctx, flat, X, y, None, True)
    assert ntc == 0 and "wide" in name
    ref, rok, spread = W.reference(F32, 160, 700, NT, False)
    assert np.array_equal(ok, rok)


# ---- 3. a loss routine, minibatches, an LDS module on a wide dataset ------------------------
def test_huber_weighted_runs_as_tree_code(gpu_ctx):
    loss = srhip.HuberLoss(1.0)
    o, trees, flat, X, y, w = W.problem(F32, 160, 700, NT)
    losses, ok, ntc, name, _, _ = run(gpu_ctx, flat, X, y, w, True, loss=loss)
    assert ntc >= 290 and name == "sr_jit_eval_dlpw", (ntc, name)
    with np.errstate(all="ignore"):
        _, ref, rok = oracle.eval_loss_batch(flat, X, y, w, loss.kind, loss.params, dtype=F32)
        spread = loss_spread(trees, o, X, y, w, F32, loss=loss) / float(w.astype(np.float64).sum())
    check_against(losses, ok, ref, rok, spread, 225, "Huber(1.0) weighted")


def test_shared_row_idx_with_repeated_indices(gpu_ctx):
    o, trees, flat, X, y, w = W.problem(F32, 160, 700, NT)
    idx = np.random.default_rng(24).integers(0, 700, 300)
    idx[:40] = idx[40:80]  # repeated indices
    for weights in (None, w):
        losses, ok, ntc, name, _, _ = run(gpu_ctx, flat, X, y, weights, True, row_idx=idx)
        assert ntc >= 290 and name.startswith("sr_jit_eval_dlp"), (ntc, name)
        with np.errstate(all="ignore"):
            _, rl, rok = oracle.eval_loss_batch(flat, X, y, weights, row_idx=idx, dtype=F32)
        wv = None if weights is None else weights[idx]
        sp = loss_spread(trees, o, X[:, idx], y[idx], wv, F32) / (len(idx) if wv is None else wv.sum())
        check_against(losses, ok, rl, rok, sp, 200, f"shared row_idx weighted={weights is not None}")


def test_flagged_lds_module_keeps_its_tree_code_on_a_wide_dataset(gpu_ctx):
    """Trees that read features 1..20 on the 160-feature dataset: the module is the LDS one
    (no candidate reads a feature from 63 on), and with the flag it stays in use."""
    o, trees, flat, X, y, w = W.problem(F32, 160, 700, NT, read=20)
    losses, ok, ntc, name, _, prog = run(gpu_ctx, flat, X, y, None, True)
    assert ntc >= 290 and name == "sr_jit_eval_dlp", (ntc, name)
    li, oki, ntci, namei, _, _ = run(gpu_ctx, flat, X, y, None, False)
    assert ntci == 0 and "wide" in namei
    # the same module on X[:20], where every kernel's tile fits
    ds20 = srhip.DeviceDataset(gpu_ctx, np.ascontiguousarray(X[:20]), y)
    s20, wsum, ok20 = prog.eval_loss(ds20, L2)
    assert gpu_ctx.last_tree_code() == ntc
    with np.errstate(all="ignore"):
        _, ref, rok = oracle.eval_loss_batch(flat, X, y, None, dtype=F32)
        spread = loss_spread(trees, o, X, y, None, F32) / 700.0
    assert np.array_equal(ok, rok) and np.array_equal(oki, rok) and np.array_equal(np.asarray(ok20).astype(bool), rok)
    m = ok & np.isfinite(ref)
    assert m.sum() >= 225
    assert_close_conditioned(losses[m], ref[m], spread[m], rtol=1e-5, msg="flagged LDS module")
    assert_close_conditioned((s20 / wsum).astype(F32)[m], ref[m], spread[m], rtol=1e-5, msg="flagged LDS module, X[:20]")


# ---- 4. new constants, device groups --------------------------------------------------------
def test_after_set_constants_the_results_are_the_oracles_at_the_new_constants(gpu_ctx):
    """Wide code holds its constants as literals and memory-constant code is never wide: the
    program runs in the (wide) interpreter from its first new constant set on."""
    o, trees, flat, X, y, w = W.problem(F32, 160, 700, NT)
    new = (np.asarray(flat.consts, dtype=np.float64) * 1.25 + 0.125).astype(F32)
    fresh = srhip.node.FlatTrees(flat.node_off, flat.kind, flat.arg, flat.const_off, new, flat.nodes)
    prog = srhip.Program(gpu_ctx, flat, F32, wide_tree_code=True)
    ds = srhip.DeviceDataset(gpu_ctx, X, y)
    prog.eval_loss(ds, L2)
    assert gpu_ctx.last_tree_code() >= 290
    prog.set_constants(new)
    s, wsum, ok = prog.eval_loss(ds, L2)
    assert gpu_ctx.last_tree_code() == 0 and "wide" in gpu_ctx.last_kernel_name()
    ok = np.asarray(ok).astype(bool)
    with np.errstate(all="ignore"):
        _, ref, rok = oracle.eval_loss_batch(fresh, X, y, None, dtype=F32)
        spread = loss_spread_flat(fresh, X, y, None, F32, srhip.L2DistLoss()) / 700.0
    assert np.array_equal(ok, rok), np.flatnonzero(ok != rok)
    m = ok & np.isfinite(ref)
    print(f"after set_constants: {int(m.sum())} trees compared")
    assert m.sum() >= 200
    assert_close_conditioned((s / wsum).astype(F32)[m], ref[m], spread[m], rtol=1e-5, msg="after set_constants")


def test_device_group_program_with_the_flag(gpu_ctx):
    o, trees, flat, X, y, w = W.problem(F32, 160, 700, NT)
    ref, rok, spread = W.reference(F32, 160, 700, NT, True)
    with srhip.DeviceGroup([0]) as g:
        gds = g.dataset(X, y, w)
        prog = g.program(flat, F32, wide_tree_code=True)
        losses, ok = srhip.eval_loss_batch_ok(trees, gds, o, program=prog)
        ntc = g.context(0).last_tree_code()
        with pytest.raises(SrhipError):
            g.program(flat, F32, flags=8)
    assert ntc >= 290, ntc
    check_against(losses, ok, ref, rok, spread, 225, "DeviceGroup([0])")
