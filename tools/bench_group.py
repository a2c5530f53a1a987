"""Cost of the device-group layer (DESIGN.md §5 "Device groups"); appends one JSON record per
row count to the list in --out (profiles/group_timing.json holds DESIGN.md's measurements).

Workload: config #2's shape (4096 trees x --rows x 5 features, Float32, L2). Compared, on the
same library build and in one process: Program.eval_loss on one context against
GroupProgram.eval_loss on the groups [0], [0, 0] and [0, 0, 0, 0] — members that share one
card, so this prices the fan-out to the driver threads, the events, the combine kernel and the
single wait, not a speed-up — and, where a second device is visible, on [0, 1]. The runs are
alternated: every repetition times one call of each configuration in turn. Reported per
configuration: the median wall time of a call and the median of the evaluation kernels' time
(HIP events, srhip_last_kernel_time; for a group summed over its members)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "symbolicregression.jl_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True, help="JSON file holding the list of records; created if missing")
    ap.add_argument("--label", default="")
    ap.add_argument("--ntrees", type=int, default=4096)
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 125_000])
    ap.add_argument("--nfeat", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import srhip
    from srhip import constants as K

    T = np.float32
    L2 = K.LOSS["L2"]
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    trees = srhip.random_population(args.ntrees, o, args.nfeat, T, seed=1000, maxsize=30)
    flat = srhip.flatten(trees, o, dtype=T)
    ndevices = srhip.device_count()
    members = [[0], [0, 0], [0, 0, 0, 0]] + ([[0, 1]] if ndevices >= 2 else [])
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for rows in args.rows:
        rng = np.random.default_rng(0)
        X = rng.standard_normal((args.nfeat, rows), dtype=T)
        y = (2 * np.cos(X[3]) + X[0] * X[0] - 2).astype(T)
        ctx = srhip.get_context(0)
        ds = srhip.DeviceDataset(ctx, X, y)
        prog = srhip.Program(ctx, flat, T)
        groups = [srhip.DeviceGroup(m) for m in members]
        gds = [g.dataset(X, y) for g in groups]
        gprog = [g.program(flat, T) for g in groups]
        gctx = [[g.context(k) for k in range(g.ndev)] for g in groups]

        def single():
            t0 = time.perf_counter()
            r = prog.eval_loss(ds, L2)
            return (time.perf_counter() - t0) * 1e3, ctx.last_kernel_time()[0], r

        def group(i):
            t0 = time.perf_counter()
            r = gprog[i].eval_loss(gds[i], L2)
            wall = (time.perf_counter() - t0) * 1e3
            return wall, sum(c.last_kernel_time()[0] for c in gctx[i]), r

        names = ["single"] + ["group" + str(m).replace(" ", "") for m in members]
        calls = [single] + [lambda i=i: group(i) for i in range(len(groups))]
        wall = {n: [] for n in names}
        kern = {n: [] for n in names}
        ref = None
        for rep in range(args.warmup + args.reps):
            for n, f in zip(names, calls):  # alternated
                w, k, r = f()
                if rep >= args.warmup:
                    wall[n].append(w)
                    kern[n].append(k)
                if n == "single":
                    ref = r
                elif n == "group[0]":  # one member: the single-context result, bit for bit
                    assert np.array_equal(r[2], ref[2]) and np.array_equal(r[0][r[2]], ref[0][ref[2]])
                else:
                    assert np.array_equal(r[2], ref[2])
        rec = dict(label=args.label, ntrees=args.ntrees, rows=rows, nfeat=args.nfeat, dtype="f32", loss="L2",
                   reps=args.reps, warmup=args.warmup, devices_visible=ndevices,
                   tree_code=[c.last_tree_code() for c in gctx[1]],
                   configs={n: dict(wall_ms=wall[n], wall_ms_median=float(np.median(wall[n])),
                                    kernel_ms_sum_median=float(np.median(kern[n]))) for n in names})
        base = rec["configs"]["single"]["wall_ms_median"]
        for n in names[1:]:
            rec["configs"][n]["wall_minus_single_ms"] = rec["configs"][n]["wall_ms_median"] - base
        recs = json.loads(out.read_text()) if out.exists() else []
        recs.append(rec)
        out.write_text(json.dumps(recs, indent=1) + "\n")
        print(json.dumps(rec))
        for g in groups:
            g.close()


if __name__ == "__main__":
    main()
