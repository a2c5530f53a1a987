"""Timing of the wide interpreter kernels, one leg per invocation; each
appends one JSON record to the list in --out (profiles/wide_timing.json holds the records of
DESIGN.md's measurements under "wide_timing").

  price: 64 features, where both paths run: 4096 trees x 1M rows, Float32, L2, no tree code
         (SRHIP_JIT=0): kernel ms (HIP events around the evaluation launches, median of
         --reps after --warmup) with SRHIP_WIDE=1 and unset, and their ratio. Run it once per
         library build (SRHIP_LIB, --label) to compare builds, as the operand prefetch was
         compared with the plain driver.
  user:  256 features, the same batch shape, in node·row/s, against the oracle's SIMD build
         on the CPUs this job may use: the method of bench.py's cpu_baseline leg (all trees on
         the first rows, sized to about --cpu-seconds).
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT / "symbolicregression.jl_amd", ROOT / "oracle"):
    sys.path.insert(0, str(p))


def available_cpus() -> int:
    """bench.py's: the cgroup CPU quota if one is set, else the affinity mask."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = Path("/sys/fs/cgroup/cpu.max").read_text().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("leg", choices=["price", "user"])
    ap.add_argument("--out", required=True, help="JSON file holding the list of records; created if missing")
    ap.add_argument("--label", default="", help="names the library build in the record")
    ap.add_argument("--ntrees", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nfeat", type=int, default=0, help="0: 64 (price), 256 (user)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--cpu-threads", type=int, default=0, help="0: every CPU this job may use")
    args = ap.parse_args()
    nfeat = args.nfeat or (64 if args.leg == "price" else 256)

    os.environ["SRHIP_JIT"] = "0"  # read when a program is built: interpreted
    import srhip
    from srhip import constants as K

    T = np.float32
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    rng = np.random.default_rng(0)
    X = rng.standard_normal((nfeat, args.rows), dtype=T)
    y = (2 * np.cos(X[nfeat - 1]) + X[0] * X[0] - 2).astype(T)
    trees = srhip.random_population(args.ntrees, o, nfeat, T, seed=1000, maxsize=30)
    flat = srhip.flatten(trees, o, dtype=T)
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    prog = srhip.Program(ctx, flat, T)
    _, total_nodes, _ = prog.info()
    node_rows = float(total_nodes) * args.rows

    def kernel_ms(wide):
        if wide is None:
            os.environ.pop("SRHIP_WIDE", None)
        else:
            os.environ["SRHIP_WIDE"] = wide
        ms, wall = [], []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            prog.eval_loss(ds, K.LOSS["L2"])
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                ms.append(ctx.last_kernel_time()[0])
                wall.append(dt)
        os.environ.pop("SRHIP_WIDE", None)
        return dict(kernel=ctx.last_kernel_name(), kernel_ms=ms, kernel_ms_median=float(np.median(ms)),
                    wall_ms_median=float(np.median(wall)), tree_code=ctx.last_tree_code())

    rec = dict(leg=args.leg, label=args.label, lib=str(srhip._lib.LIB_PATH.name), nfeat=nfeat, ntrees=args.ntrees,
               rows=args.rows, dtype="f32", loss="L2", total_nodes=int(total_nodes), reps=args.reps,
               warmup=args.warmup)
    if args.leg == "price":
        rec["lds"] = kernel_ms(None)
        rec["wide"] = kernel_ms("1")
        rec["lds_again"] = kernel_ms(None)  # alternated: the LDS path before and after
        rec["ratio_wide_over_lds"] = rec["wide"]["kernel_ms_median"] / rec["lds"]["kernel_ms_median"]
    else:
        g = kernel_ms(None)
        rec["gpu"] = g
        rec["gpu_node_rows_per_s_kernel"] = node_rows / (g["kernel_ms_median"] * 1e-3)
        rec["gpu_node_rows_per_s_wall"] = node_rows / (g["wall_ms_median"] * 1e-3)
        import oracle

        threads = args.cpu_threads or available_cpus()

        def run_cpu(nrows):
            t_ = time.perf_counter()
            oracle.eval_loss_batch(flat, X[:, :nrows], y[:nrows], dtype=T, nthreads=threads, variant="simd")
            return time.perf_counter() - t_, float(flat.nodes.sum()) * nrows

        probe = min(args.rows, 10_000)
        dt, nr = run_cpu(probe)
        nrows = int(min(args.rows, max(probe, probe * args.cpu_seconds / max(dt, 1e-3))))
        dt, nr = run_cpu(nrows)
        rec["cpu"] = dict(node_rows_per_s=nr / dt, threads=threads, rows=nrows, seconds=dt,
                          what="oracle simd build, OpenMP over trees")
        rec["gpu_over_cpu_kernel"] = rec["gpu_node_rows_per_s_kernel"] / rec["cpu"]["node_rows_per_s"]
        rec["gpu_over_cpu_wall"] = rec["gpu_node_rows_per_s_wall"] / rec["cpu"]["node_rows_per_s"]
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    recs = json.loads(out.read_text()) if out.exists() else []
    recs.append(rec)
    out.write_text(json.dumps(recs, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
