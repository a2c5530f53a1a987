"""The calls of tests/test_jit_tail_trees_gpu.py, run in a child process:

    python jit_tail_trees_cases.py VARIANT [VARIANT ...]

prints one JSON line {variant: {setting: result}}. A setting is "S{S}-n{n}"
(SRHIP_JIT_TAIL_TREES=S, SRHIP_JIT_TAIL_RG=n: each tree group of the last n row
groups run by S workgroups), "S1" (no tree group split) or "default" (neither
knob set), with "-r{mode}" appended where SRHIP_JIT_ROTATE is set. The knobs are
read per launch, so one process runs every setting of a variant on one program.
Each result carries the launch's geometry (Context.last_loss_launch). The
parent process chooses the tree groups with SRHIP_TARGET_WG (read once per
process): 92 gives 22 groups of 14 list positions, 308 slots for the 300 trees.

The batch: 300 trees of config #2's operators on 5 features, 3·1024 + 300 rows
(four row groups, the last ragged). 296 seeded random trees (about a quarter
fail on some row) and four hand-made ones in the middle of the list:
  x3 / (x1 − x1)   fails on every row;
  x3 / x5          fails on row 3300 only, a late row of the last row group
                   (x5 is zero there; the random trees dividing by x5 fail
                   there too);
  x3 / x2          x2 = 2⁻¹⁰⁰ on row 0: the quotient leaves the FAST division's
                   range, so the first tile of the first row group is redone
                   with the PRECISE routines;
  x1 · 1e7         under the Periodic loss its residual leaves the routine's
                   range: the tree is handed back to the interpreter.
"""
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "symbolicregression.jl_amd"))

NTREES, ROWS = 300, 3 * 1024 + 300
LATE_ROW = 3300
TAIL_RG, TAIL_TREES = (1, 2, 4), (2, 4, 8)
CFG2 = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
HAND = {"every_row": NTREES // 2, "late_row": NTREES // 2 + 1, "redo": NTREES // 2 + 2, "bail": NTREES // 2 + 3}


def problem(weighted=False):
    import srhip

    F32 = np.float32
    o = srhip.Options(**CFG2)
    N = srhip.Node
    trees = srhip.random_population(NTREES - 4, o, 5, np.float32, seed=1300)
    hand = [o.make_binary("/", N(feature=3), o.make_binary("-", N(feature=1), N(feature=1))),
            o.make_binary("/", N(feature=3), N(feature=5)),
            o.make_binary("/", N(feature=3), N(feature=2)),
            o.make_binary("*", N(feature=1), N(val=F32(1e7)))]
    trees = trees[: NTREES // 2] + hand + trees[NTREES // 2:]
    rng = np.random.default_rng(NTREES + ROWS)
    X = rng.standard_normal((5, ROWS)).astype(F32)
    X[4, LATE_ROW] = 0
    X[1, 0] = F32(2.0 ** -100)
    y = (F32(2) * np.cos(X[3]) + X[0] * X[0] - F32(2)).astype(F32)
    w = rng.uniform(0.5, 2.0, ROWS).astype(F32) if weighted else None
    return o, trees, X, y, w


def settings(rotate=(None,)):
    out = []
    for r in rotate:
        rk = {} if r is None else {"SRHIP_JIT_ROTATE": str(r)}
        tag = "" if r is None else f"-r{r}"
        out.append(("default" + tag, dict(rk)))
        out.append(("S1" + tag, dict(rk, SRHIP_JIT_TAIL_TREES="1")))
        for S in TAIL_TREES:
            for n in TAIL_RG:
                out.append((f"S{S}-n{n}{tag}", dict(rk, SRHIP_JIT_TAIL_TREES=str(S), SRHIP_JIT_TAIL_RG=str(n))))
    return out


class env:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def record(ctx, prog, res):
    sums, wsum, ok = res
    bailed, redone = ctx.last_jit_events()
    info = prog.jit_info()
    return dict(sums=np.asarray(sums, np.float64).tobytes().hex(), ok=np.asarray(ok, np.uint8).tobytes().hex(),
                wsum=float(wsum), kernel=ctx.last_kernel_name(), launches=ctx.last_kernel_time()[1],
                tree_code=ctx.last_tree_code(), bailed=bailed, redone=redone, geometry=ctx.last_loss_launch(),
                info={k: info[k] for k in ("ntrees", "nfast", "code_bytes")})


def variant(name):
    import srhip
    from srhip import constants as K

    weighted = name == "weighted"
    o, trees, X, y, w = problem(weighted)
    flat = srhip.flatten(trees, o, dtype=np.float32)
    ctx = srhip.get_context(0)
    build = {"SRHIP_JIT": "1", "SRHIP_JIT_STICKY_TREE": "0"}  # sticky mark: which tiles run PRECISE depends on the order
    if name == "plain":
        build["SRHIP_JIT_PREFETCH"] = "0"
    if name == "plain_order":  # blocks in launch order, not dealt over the XCDs (read per launch)
        build["SRHIP_RG_XCD"] = "0"
    loss, params = K.LOSS["L2"], None
    if name == "periodic_bail":
        pl = srhip.PeriodicLoss(2.0)
        loss, params = pl.kind, pl.params
    out = {}
    with env(build):
        ds = srhip.DeviceDataset(ctx, X, y, w)
        if name == "two_contexts":  # a program of a second context on the first context's dataset
            other = srhip.engine.Context(0)
            prog = srhip.Program(other, flat, np.float32)
            rctx = other
        else:
            prog = srhip.Program(ctx, flat, np.float32, varying_constants=False)
            rctx = ctx
        if name == "set_constants":  # new constants: the tree code reads them from memory from now on
            c = np.array(flat.consts, dtype=np.float32, copy=True)
            c *= np.float32(1.25)
            prog.set_constants(c)
        for tag, kv in settings((0, 1, 2) if name == "rotate" else (None,)):
            with env(kv):
                out[tag] = record(rctx, prog, prog.eval_loss(ds, loss, params))
    return out


def main(names):
    print(json.dumps({n: variant(n) for n in names}))


if __name__ == "__main__":
    main(sys.argv[1:])
