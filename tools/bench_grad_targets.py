"""Constant optimisation of a multi-output population in one fused call against the
same trees optimised output by output on the views:
optimize_constants_batch(mds, trees, targets=..., fused=True) and K calls of
optimize_constants_batch(mds.target(k), ...) with each group's slice of the same
start noise, alternated in one process (Float32, L2, config #2's operators, 5
features, K = 4 targets, 8 BFGS iterations, 1 + 2 starts per tree). The K view
calls are what a caller could do before the fused call existed. Each side is timed
as the median of `--steps` calls after `--warmup`, the pair repeated `--repeats`
times for the spread. Every call works on fresh copies of the trees. The device
has to be there; there is no fallback. Prints one JSON line per case.

A case is per_target:rows:batch_size; batch_size 0 runs on all rows.

Usage: bench_grad_targets.py [--cases 33:10000:0,33:100000:0,256:100000:0,33:100000:50,33:100000:1000]
                             [--steps 7] [--warmup 3] [--repeats 3] [--out FILE]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "symbolicregression.jl_amd"))
import srhip  # noqa: E402
from srhip.constant_optimization import last_profile, start_noise  # noqa: E402

NFEAT, K = 5, 4


def timed(call, steps, warmup):
    """(median seconds, result of the last call)."""
    for _ in range(warmup):
        call()
    runs = []
    for _ in range(steps):
        t0 = time.perf_counter()
        res = call()
        runs.append(time.perf_counter() - t0)
    runs.sort()
    return runs[len(runs) // 2], res


def case(per_target, rows, bs, args):
    if srhip.device_count() == 0:
        raise SystemExit("bench_grad_targets: no HIP device")
    T = np.float32
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    rng = np.random.default_rng(1)
    X = rng.standard_normal((NFEAT, rows)).astype(T)
    Y = np.stack([2 * np.cos(X[3]) + X[0] ** 2 - 2, X[1] * X[2] + 0.5, np.exp(0.3 * X[4]) - X[0],
                  X[0] - 0.5 * X[2] * X[2]]).astype(T)
    mds = srhip.MultiDataset(X, Y)
    n = K * per_target
    trees = srhip.random_population(n, o, NFEAT, T, seed=0)
    tg = (np.arange(n) % K).astype(np.int32)
    flat = srhip.flatten(trees, o, dtype=T)
    nre = o.optimizer_nrestarts
    noise = start_noise(flat, nre, np.random.default_rng(0))
    noff = nre * np.asarray(flat.const_off, dtype=np.int64)
    idx = np.random.default_rng(2).integers(0, rows, (n, bs)) if bs else None
    groups = [np.flatnonzero(tg == k) for k in range(K)]
    sub_noise = [np.concatenate([noise[noff[t]:noff[t + 1]] for t in g]) for g in groups]
    ctx = mds.device().ctx
    prof = {}

    def fused():
        r = srhip.optimize_constants_batch(mds, [t.copy() for t in trees], o, noise=noise, row_idx=idx, targets=tg,
                                           fused=True)
        prof["fused"] = last_profile()
        return r

    def views():
        out = []
        for k, g in enumerate(groups):
            out.append(srhip.optimize_constants_batch(mds.target(k), [trees[t].copy() for t in g], o,
                                                      noise=sub_noise[k], row_idx=None if idx is None else idx[g]))
        prof["views_last"] = last_profile()
        return out

    pairs = []
    for _ in range(args.repeats):
        tf, rf = timed(fused, args.steps, args.warmup)
        fused_kernel, fused_code = ctx.last_kernel_name(), ctx.last_tree_code()
        tv, rv = timed(views, args.steps, args.warmup)
        pairs.append(dict(fused_s=tf, views_s=tv, ratio=tv / tf, fused_last_kernel=fused_kernel,
                          fused_tree_code=fused_code, views_last_kernel=ctx.last_kernel_name(),
                          views_tree_code=ctx.last_tree_code()))
    out = dict(tool="bench_grad_targets", per_target=per_target, ntargets=K, ntrees=n, rows=rows, batch_size=bs,
               nfeat=NFEAT, dtype="float32", loss="L2", steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               fused_s=[p["fused_s"] for p in pairs], views_s=[p["views_s"] for p in pairs],
               ratio=[p["ratio"] for p in pairs],
               fused_below_views=max(p["fused_s"] for p in pairs) < min(p["views_s"] for p in pairs),
               fused_converged=int(rf.converged.sum()), views_converged=int(sum(r.converged.sum() for r in rv)),
               fused_profile=prof["fused"], views_last_profile=prof["views_last"], pairs=pairs)
    print(json.dumps(out))
    sys.stdout.flush()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="33:10000:0,33:100000:0,256:100000:0,33:100000:50,33:100000:1000",
                    help="per_target:rows:batch_size (0: all rows), comma separated")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the cases as one JSON document")
    args = ap.parse_args()
    res = [case(*(int(v) for v in c.split(":")), args) for c in args.cases.split(",")]
    if args.out:
        Path(args.out).write_text(json.dumps(dict(cases=res), indent=1) + "\n")


if __name__ == "__main__":
    main()
