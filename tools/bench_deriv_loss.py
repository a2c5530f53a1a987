"""Timing record of the derivative-objective kernel:
srhip_eval_loss_deriv on 4096 random trees x 1M rows x 5 features, Float32, L2, for
ndir = 1, 2 and 5 directions, as kernel milliseconds (srhip_last_kernel_time, the
device events around the main kernels of a call), median of `--steps` calls after
`--warmup`. Each is set beside
  (a) the interpreter's plain loss kernel on the same trees and rows
      (Program(..., interpreted=True).eval_loss): the cost of the value channel alone;
  (c) the same forward-mode interpreter carrying constant tangents: GRAD_LOSS on the
      same trees and rows without tree code (eval_loss_grad_targets on one column),
      with its work items per pass (1, 2, 4 tangents, deep), so that the cost per work
      item can be set beside the derivative mode's (one item per tree and group);
  (b) the only way to the same numbers without the fused call: eval_tree_array +
      eval_diff_tree_array per direction and a host reduction, wall clock, at
      256 trees x 100k rows, where its per-row output still fits, against the fused
      call's wall clock on the same trees (program built per call on both sides).
The device has to be there; there is no fallback. Writes one JSON document.

Usage: bench_deriv_loss.py [--trees 4096] [--rows 1000000] [--steps 10] [--warmup 3]
                           [--small 256:100000] [--out profiles/deriv_loss_timing.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "symbolicregression.jl_amd"))
import srhip  # noqa: E402
from srhip import constants as K  # noqa: E402
from srhip.engine import MultiDeviceDataset, Program  # noqa: E402

NFEAT = 5
DIRS = {1: [1], 2: [1, 4], 5: [1, 2, 3, 4, 5]}


def median_kernel_ms(call, ctx, steps, warmup):
    """(median, min, max) of the call's kernel milliseconds, and its launches."""
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(steps):
        call()
        t, n = ctx.last_kernel_time()
        ms.append(t)
    ms.sort()
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], launches=n)


def median_wall_s(call, steps, warmup):
    for _ in range(warmup):
        call()
    s = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        s.append(time.perf_counter() - t0)
    s.sort()
    return dict(median_s=s[len(s) // 2], min_s=s[0], max_s=s[-1])


def problem(ntrees, rows):
    T = np.float32
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    X = np.random.default_rng(1).standard_normal((NFEAT, rows)).astype(T)
    y = (2 * np.cos(X[3]) + X[0] ** 2 - 2).astype(T)
    G = np.stack([2 * X[0], np.zeros(rows, T), np.zeros(rows, T), -2 * np.sin(X[3]), np.zeros(rows, T)]).astype(T)
    return o, srhip.random_population(ntrees, o, NFEAT, T, seed=0), X, y, G


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", default="256:100000", help="trees:rows of comparison (b)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "deriv_loss_timing.json"))
    args = ap.parse_args()
    if srhip.device_count() == 0:
        raise SystemExit("bench_deriv_loss: no HIP device")
    T = np.float32
    ctx = srhip.get_context(0)
    o, trees, X, y, G = problem(args.trees, args.rows)
    flat = srhip.flatten(trees, o, dtype=T)
    prog = Program(ctx, flat, T, interpreted=True)
    # (a) the value channel alone: the interpreter's loss kernel
    ds1 = srhip.DeviceDataset(ctx, X, y)
    plain = median_kernel_ms(lambda: prog.eval_loss(ds1, K.LOSS["L2"]), ctx, args.steps, args.warmup)
    plain["kernel"] = ctx.last_kernel_name()
    # (c) the forward-mode interpreter with constant tangents on the same trees
    mds1 = MultiDeviceDataset(ctx, X, y[None, :])
    tg0 = np.zeros(args.trees, dtype=np.int32)
    grad = median_kernel_ms(lambda: prog.eval_loss_grad_targets(mds1, K.LOSS["L2"], tg0), ctx, args.steps, args.warmup)
    grad.update(kernel=ctx.last_kernel_name(), items_per_pass=list(prog.pass_info()["grad_items"]))
    grad["ms_per_1000_items"] = 1000 * grad["median_ms"] / max(1, sum(grad["items_per_pass"]))
    del mds1
    cases = []
    for ndir, dirs in DIRS.items():
        Y = np.concatenate([y[None, :], G[[d - 1 for d in dirs]]])
        mds = MultiDeviceDataset(ctx, X, Y)
        d0 = [d - 1 for d in dirs]
        r = median_kernel_ms(lambda: prog.eval_loss_deriv(mds, K.LOSS["L2"], d0), ctx, args.steps, args.warmup)
        sums, wsum, ok = prog.eval_loss_deriv(mds, K.LOSS["L2"], d0)
        groups = (ndir + 3) // 4
        r.update(ndir=ndir, directions=dirs, kernel=ctx.last_kernel_name(), tangent_groups=groups,
                 launch=ctx.last_loss_launch(), ok=int(ok.sum()), ratio_to_plain=r["median_ms"] / plain["median_ms"],
                 ratio_to_plain_per_group=r["median_ms"] / plain["median_ms"] / groups,
                 items=args.trees * groups, ms_per_1000_items=1000 * r["median_ms"] / (args.trees * groups))
        cases.append(r)
        print(json.dumps(r))
        sys.stdout.flush()
        del mds
    # (b) per-row derivatives and a host reduction, against the fused call, wall clock
    st, sr = (int(v) for v in args.small.split(":"))
    o, strees, Xs, ys, Gs = problem(st, sr)
    small = []
    for ndir, dirs in DIRS.items():
        dds = srhip.DerivativeDataset(Xs, ys, Gs[[d - 1 for d in dirs]], dirs)

        def host():
            val, ok = srhip.eval_tree_array(strees, Xs, o)
            out = np.empty((st, 1 + ndir))
            out[:, 0] = ((val.astype(np.float64) - ys) ** 2).sum(axis=1)
            for j, d in enumerate(dirs):
                _, g, _ = srhip.eval_diff_tree_array(strees, Xs, o, d)
                out[:, 1 + j] = ((np.asarray(g, dtype=np.float64) - Gs[d - 1]) ** 2).sum(axis=1)
            return out, ok

        fused = median_wall_s(lambda: srhip.eval_deriv_loss_batch(strees, dds, o), args.steps, args.warmup)
        per_row = median_wall_s(host, max(3, args.steps // 3), 1)
        rec = dict(ndir=ndir, trees=st, rows=sr, fused_wall_s=fused, per_row_wall_s=per_row,
                   ratio=per_row["median_s"] / fused["median_s"])
        small.append(rec)
        print(json.dumps(rec))
        sys.stdout.flush()
    doc = dict(tool="bench_deriv_loss", dtype="float32", loss="L2", nfeat=NFEAT, trees=args.trees, rows=args.rows,
               steps=args.steps, warmup=args.warmup, kernel_ms_source="srhip_last_kernel_time (device events)",
               plain_loss_interpreted=plain, grad_loss_interpreted=grad, deriv=cases, per_row_comparison=small)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
