"""Timing record of the constant gradients of a derivative objective:
srhip_eval_loss_grad_deriv on 4096 random trees x 1M rows x 5 features, Float32, L2, for
ndir = 1 and 2, as kernel milliseconds (srhip_last_kernel_time), median of `--steps` calls
after `--warmup`, with min and max. Yardsticks, measured in the same process:
  (a) the first-order kernel of the objective, grad_kernel_deriv (srhip_eval_loss_deriv) on
      the same trees, per 1000 work items;
  (b) GRAD_LOSS on the same trees without tree code (eval_loss_grad_targets on one column),
      per 1000 work items;
  (c) central differences through srhip_eval_loss_deriv: 2·nconst re-evaluations per tree,
      which is what an optimiser without a gradient pays. Measured as the kernel time of one
      srhip_eval_loss_deriv call on a program that holds every tree 2·nconst(tree) times
      (the perturbed copies: the same work as the re-evaluations, in one launch, which favours
      the yardstick), capped at `--fd-trees` trees and scaled to the full batch by work items.
and one optimize_constants_deriv_batch run of 256 members x 100k rows under the objective (wall time
and srhip_constopt_profile's split). The device has to be there. Writes one JSON document.

Usage: bench_deriv_grad.py [--trees 4096] [--rows 1000000] [--steps 10] [--warmup 3]
                           [--fd-trees 1024] [--out profiles/deriv_grad_timing.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "symbolicregression.jl_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import srhip  # noqa: E402
from bench_deriv_loss import median_kernel_ms, problem  # noqa: E402
from srhip import constants as K  # noqa: E402
from srhip.engine import MultiDeviceDataset, Program  # noqa: E402

DIRS = {1: [1], 2: [1, 4]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fd-trees", type=int, default=1024)
    ap.add_argument("--opt", default="256:100000", help="members:rows of the optimiser run")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "deriv_grad_timing.json"))
    args = ap.parse_args()
    if srhip.device_count() == 0:
        raise SystemExit("bench_deriv_grad: no HIP device")
    T = np.float32
    L2 = K.LOSS["L2"]
    ctx = srhip.get_context(0)
    o, trees, X, y, G = problem(args.trees, args.rows)
    flat = srhip.flatten(trees, o, dtype=T)
    nconst = np.diff(flat.const_off)
    prog = Program(ctx, flat, T, interpreted=True)
    mds1 = MultiDeviceDataset(ctx, X, y[None, :])
    tg0 = np.zeros(args.trees, dtype=np.int32)
    grad = median_kernel_ms(lambda: prog.eval_loss_grad_targets(mds1, L2, tg0), ctx, args.steps, args.warmup)
    grad.update(kernel=ctx.last_kernel_name(), items_per_pass=list(prog.pass_info()["grad_items"]))
    grad["ms_per_1000_items"] = 1000 * grad["median_ms"] / max(1, sum(grad["items_per_pass"]))
    del mds1
    # the perturbed copies of the central differences, over the first fd_trees trees
    nfd = min(args.fd_trees, args.trees)
    copies = [t for i, t in enumerate(trees[:nfd]) for _ in range(2 * int(nconst[i]))]
    fdprog = Program(ctx, srhip.flatten(copies, o, dtype=T), T, interpreted=True)
    fd_scale = float(2 * nconst.sum()) / max(1, len(copies))
    cases = []
    for ndir, dirs in DIRS.items():
        Y = np.concatenate([y[None, :], G[[d - 1 for d in dirs]]])
        mds = MultiDeviceDataset(ctx, X, Y)
        d0 = [d - 1 for d in dirs]
        first = median_kernel_ms(lambda: prog.eval_loss_deriv(mds, L2, d0), ctx, args.steps, args.warmup)
        first.update(kernel=ctx.last_kernel_name(), items=args.trees,
                     ms_per_1000_items=1000 * first["median_ms"] / args.trees)
        r = median_kernel_ms(lambda: prog.eval_loss_grad_deriv(mds, L2, d0), ctx, args.steps, args.warmup)
        sums, grads, wsum, ok = prog.eval_loss_grad_deriv(mds, L2, d0)
        launch, kernel = ctx.last_loss_launch(), ctx.last_kernel_name()
        fd = median_kernel_ms(lambda: fdprog.eval_loss_deriv(mds, L2, d0), ctx, args.steps, args.warmup)
        fd_full = {k: fd[k] * fd_scale for k in ("median_ms", "min_ms", "max_ms")}
        spread = fd_full["max_ms"] - fd_full["min_ms"]
        r.update(ndir=ndir, directions=dirs, kernel=kernel,
                 launch=launch, ok=int(ok.sum()), constants=int(nconst.sum()),
                 first_order_deriv=first, central_differences=dict(measured_on_trees=nfd, copies=len(copies),
                                                                   scale_to_batch=fd_scale, measured=fd, **fd_full),
                 speedup_over_central_differences=fd_full["median_ms"] / r["median_ms"],
                 wins_by_more_than_yardstick_spread=bool(fd_full["median_ms"] - r["median_ms"] > spread))
        cases.append(r)
        print(json.dumps(r))
        sys.stdout.flush()
        del mds
    # one optimiser run under the objective
    om, orows = (int(v) for v in args.opt.split(":"))
    o2, otrees, Xs, ys, Gs = problem(om, orows)
    dds = srhip.DerivativeDataset(Xs, ys, Gs[[0]], [1])
    oo = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"],
                       loss_function=srhip.DerivativeObjective([1.0, 1.0]))
    srhip.optimize_constants_deriv_batch(dds, [t.copy() for t in otrees[:8]], oo, rng=np.random.default_rng(0))  # warm-up
    t0 = time.perf_counter()
    res = srhip.optimize_constants_deriv_batch(dds, [t.copy() for t in otrees], oo, rng=np.random.default_rng(0))
    wall = time.perf_counter() - t0
    opt = dict(members=om, rows=orows, ndir=1, wall_s=wall, converged=int(res.converged.sum()),
               profile=srhip.constant_optimization.last_profile())
    print(json.dumps(opt))
    doc = dict(tool="bench_deriv_grad", dtype="float32", loss="L2", nfeat=5, trees=args.trees, rows=args.rows,
               steps=args.steps, warmup=args.warmup, kernel_ms_source="srhip_last_kernel_time (device events)",
               grad_loss_interpreted=grad, deriv_grad=cases, optimiser_run=opt,
               not_measured=["Float64 timings", "the deep variant alone", "a search run", "Julia"])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
