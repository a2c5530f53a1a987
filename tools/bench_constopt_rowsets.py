"""Constant optimisation on per-tree row samples against the full-data optimiser
(DESIGN.md §3.16): optimize_constants_batch(..., row_idx=rows) and
optimize_constants_batch on all rows, alternated in one process on one random
population (Float32, L2, config #2's operators, 10 features, 8 BFGS iterations,
1 + 2 starts per tree), each timed as the median of `--steps` calls after
`--warmup`, the pair repeated `--repeats` times for the spread. Every call works
on fresh copies of the trees with the same start noise. The device has to be
there; there is no fallback. Prints one JSON line per case with
srhip_constopt_profile's split (program builds, set_constants, loss and gradient
calls, kernels, sample gathers, host algebra) of the median call.

Usage: bench_constopt_rowsets.py [--cases 320:100000:50,320:100000:1000,1024:1000000:1000]
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

NFEAT = 10


def timed(call, steps, warmup):
    """(median seconds, profile of the median call, result of the last call)."""
    for _ in range(warmup):
        call()
    runs = []
    for _ in range(steps):
        t0 = time.perf_counter()
        res = call()
        runs.append((time.perf_counter() - t0, last_profile()))
    runs.sort(key=lambda r: r[0])
    return runs[len(runs) // 2][0], runs[len(runs) // 2][1], res


def case(ntrees, rows, bs, args):
    if srhip.device_count() == 0:
        raise SystemExit("bench_constopt_rowsets: no HIP device")
    T = np.float32
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    rng = np.random.default_rng(1)
    X = rng.standard_normal((NFEAT, rows)).astype(T)
    y = (2 * np.cos(X[3]) + X[0] ** 2 - 2).astype(T)
    ds = srhip.Dataset(X, y)
    trees = srhip.random_population(ntrees, o, NFEAT, T, seed=0)
    noise = start_noise(srhip.flatten(trees, o, dtype=T), o.optimizer_nrestarts, np.random.default_rng(0))
    idx = np.random.default_rng(2).integers(0, rows, (ntrees, bs))  # with replacement, one sample per tree
    ctx = ds.device().ctx

    def full():
        return srhip.optimize_constants_batch(ds, [t.copy() for t in trees], o, noise=noise)

    def sampled():
        return srhip.optimize_constants_batch(ds, [t.copy() for t in trees], o, noise=noise, row_idx=idx)

    pairs = []
    for _ in range(args.repeats):
        tf, pf, rf = timed(full, args.steps, args.warmup)
        full_kernel = ctx.last_kernel_name()
        ts, ps, rs = timed(sampled, args.steps, args.warmup)
        pairs.append(dict(full_s=tf, rowsets_s=ts, ratio=tf / ts, full_profile=pf, rowsets_profile=ps,
                          full_last_kernel=full_kernel, rowsets_last_kernel=ctx.last_kernel_name(),
                          rowsets_tree_code=ctx.last_tree_code()))
    out = dict(tool="bench_constopt_rowsets", ntrees=ntrees, rows=rows, batch_size=bs, nfeat=NFEAT, dtype="float32",
               loss="L2", steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               full_s=[p["full_s"] for p in pairs], rowsets_s=[p["rowsets_s"] for p in pairs],
               ratio=[p["ratio"] for p in pairs],
               full_loss_evals=float(rf.num_evals.sum()), rowsets_loss_evals=float(rs.num_evals.sum()),
               full_converged=int(rf.converged.sum()), rowsets_converged=int(rs.converged.sum()), pairs=pairs)
    print(json.dumps(out))
    sys.stdout.flush()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="320:100000:50,320:100000:1000,1024:1000000:1000",
                    help="ntrees:rows:batch_size, comma separated")
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
