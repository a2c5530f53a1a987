"""Timing record of the objective's one-pass gradient tree code:
srhip_eval_objective_grad_deriv on 4096 random trees x 1M rows x 5 features, Float32, L2, for
ndir = 1, 2, 4, as kernel milliseconds (srhip_last_kernel_time: every launch of the call, the
interpreter's share for refused trees included), median of `--steps` calls after `--warmup`
with min and max. The flagged program and the parent's path (the same call on an unflagged
program: grad_kernel_deriv2<float>) alternate call by call in one process. Beside them:
  (a) the central-difference yardstick of tools/bench_deriv_grad.py (one srhip_eval_loss_deriv
      call on a program holding every tree 2·nconst(tree) times, capped at --fd-trees trees and
      scaled to the batch);
  (b) the dv loss tree code (srhip_eval_loss_deriv on a SRHIP_PROGRAM_DERIV_TREE_CODE program).
Bar (§3.19): the new path's median below the central differences' range. Writes one JSON document.

Usage: bench_deriv_grad_tree_code.py [--trees 4096] [--rows 1000000] [--steps 10] [--warmup 3]
                                     [--fd-trees 1024] [--out profiles/deriv_grad_tree_code_timing.json]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "symbolicregression.jl_amd"))
sys.path.insert(0, str(ROOT / "tools"))
import srhip  # noqa: E402
from bench_deriv_loss import median_kernel_ms, problem  # noqa: E402
from srhip import constants as K  # noqa: E402
from srhip.engine import MultiDeviceDataset, Program  # noqa: E402

DIRS = {1: [1], 2: [1, 4], 4: [1, 4, 2, 3]}


def stats(ms, launches):
    ms = sorted(ms)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], launches=launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fd-trees", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "deriv_grad_tree_code_timing.json"))
    args = ap.parse_args()
    if srhip.device_count() == 0:
        raise SystemExit("bench_deriv_grad_tree_code: no HIP device")
    T = np.float32
    L2 = K.LOSS["L2"]
    ctx = srhip.get_context(0)
    o, trees, X, y, G = problem(args.trees, args.rows)
    flat = srhip.flatten(trees, o, dtype=T)
    nconst = np.diff(flat.const_off)
    new = Program(ctx, flat, T, interpreted=True, deriv_grad_tree_code=True)
    old = Program(ctx, flat, T, interpreted=True)
    dv = Program(ctx, flat, T, interpreted=True, deriv_tree_code=True)
    nfd = min(args.fd_trees, args.trees)
    copies = [t for i, t in enumerate(trees[:nfd]) for _ in range(2 * int(nconst[i]))]
    fdprog = Program(ctx, srhip.flatten(copies, o, dtype=T), T, interpreted=True)
    fd_scale = float(2 * nconst.sum()) / max(1, len(copies))
    cases = []
    for ndir, dirs in DIRS.items():
        Y = np.concatenate([y[None, :], G[[d - 1 for d in dirs]]])
        mds = MultiDeviceDataset(ctx, X, Y)
        d0 = [d - 1 for d in dirs]
        coef = np.ones(1 + ndir)
        tn, to, info = [], [], {}
        for step in range(args.warmup + args.steps):  # the two paths alternate
            for name, prog, ms in (("new", new, tn), ("old", old, to)):
                sums, g, wsum, ok = prog.eval_objective_grad_deriv(mds, L2, d0, coef)
                t, n = ctx.last_kernel_time()
                if step >= args.warmup:
                    ms.append(t)
                info[name] = dict(kernel=ctx.last_kernel_name(), compiled=ctx.last_tree_code(), launches=n,
                                  ok=int(ok.sum()), finite_gradients=int(np.isfinite(g).sum()))
        r = stats(tn, info["new"]["launches"])
        r.update(ndir=ndir, directions=dirs, constants=int(nconst.sum()), **info["new"],
                 fell_back=args.trees - info["new"]["compiled"])
        r["interpreter_path"] = dict(stats(to, info["old"]["launches"]), **info["old"])
        loss = median_kernel_ms(lambda: dv.eval_loss_deriv(mds, L2, d0), ctx, args.steps, args.warmup)
        loss.update(kernel=ctx.last_kernel_name(), compiled=ctx.last_tree_code())
        fd = median_kernel_ms(lambda: fdprog.eval_loss_deriv(mds, L2, d0), ctx, args.steps, args.warmup)
        fd_full = {k: fd[k] * fd_scale for k in ("median_ms", "min_ms", "max_ms")}
        r.update(dv_loss_tree_code=loss, ratio_to_dv_loss_tree_code=r["median_ms"] / loss["median_ms"],
                 central_differences=dict(measured_on_trees=nfd, copies=len(copies), scale_to_batch=fd_scale,
                                          measured=fd, **fd_full),
                 speedup_over_interpreter_path=r["interpreter_path"]["median_ms"] / r["median_ms"],
                 speedup_over_central_differences=fd_full["median_ms"] / r["median_ms"],
                 below_central_differences_range=bool(r["median_ms"] < fd_full["min_ms"]))
        cases.append(r)
        print(json.dumps(r))
        sys.stdout.flush()
        del mds
    doc = dict(tool="bench_deriv_grad_tree_code", dtype="float32", loss="L2", nfeat=5, trees=args.trees, rows=args.rows,
               steps=args.steps, warmup=args.warmup, kernel_ms_source="srhip_last_kernel_time (device events)",
               cases=cases, not_measured=["weighted timings", "other losses", "module build time", "Julia"])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
