"""Timing of wide loss tree code (SRHIP_PROGRAM_WIDE_TREE_CODE) against the
wide interpreter on tools/bench_wide.py's user batch: 256 features, 4096 trees x 1M rows,
Float32, L2. One process holds one program per variant and alternates them call by call:
kernel ms (HIP events around every evaluation launch of the call, the interpreter passes for
the trees without code included), --reps samples each after --warmup rounds.

Variants: "off" (no flag: the wide interpreter) and one flagged program per window depth of
--xdepth (SRHIP_JIT_XDEPTH is read per build; the first one listed is the one reported as
"on"). Appends one JSON record to the list in --out (profiles/wide_tree_code_timing.json).
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "symbolicregression.jl_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--label", default="")
    ap.add_argument("--ntrees", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--nfeat", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--xdepth", default="", help="comma-separated window depths; empty: the default only")
    args = ap.parse_args()

    import srhip
    from srhip import constants as K

    T = np.float32
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    rng = np.random.default_rng(0)
    X = rng.standard_normal((args.nfeat, args.rows), dtype=T)
    y = (2 * np.cos(X[args.nfeat - 1]) + X[0] * X[0] - 2).astype(T)
    trees = srhip.random_population(args.ntrees, o, args.nfeat, T, seed=1000, maxsize=30)
    flat = srhip.flatten(trees, o, dtype=T)
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)

    progs = {"off": srhip.Program(ctx, flat, T)}
    depths = [d for d in args.xdepth.split(",") if d != ""]
    for d in depths or [None]:
        if d is None:
            os.environ.pop("SRHIP_JIT_XDEPTH", None)
        else:
            os.environ["SRHIP_JIT_XDEPTH"] = d
        progs["on" if d is None else f"on_depth{d}"] = srhip.Program(ctx, flat, T, wide_tree_code=True)
    os.environ.pop("SRHIP_JIT_XDEPTH", None)
    _, total_nodes, _ = progs["off"].info()
    node_rows = float(total_nodes) * args.rows

    res = {k: dict(kernel_ms=[], wall_ms=[]) for k in progs}
    sums = {}
    for i in range(args.warmup + args.reps):
        for k, p in progs.items():
            t0 = time.perf_counter()
            s, _, ok = p.eval_loss(ds, K.LOSS["L2"])
            dt = (time.perf_counter() - t0) * 1e3
            r = res[k]
            r["kernel"], r["tree_code"], r["jit_events"] = ctx.last_kernel_name(), ctx.last_tree_code(), list(ctx.last_jit_events())
            sums[k] = (np.array(s), np.array(ok))
            if i >= args.warmup:
                r["kernel_ms"].append(ctx.last_kernel_time()[0])
                r["wall_ms"].append(dt)
    for k, r in res.items():
        r["kernel_ms_median"] = float(np.median(r["kernel_ms"]))
        r["kernel_ms_min"] = float(np.min(r["kernel_ms"]))
        r["wall_ms_median"] = float(np.median(r["wall_ms"]))
        r["node_rows_per_s_kernel"] = node_rows / (r["kernel_ms_median"] * 1e-3)
        r["jit_info"] = progs[k].jit_info()
        # agreement with the interpreter: did_succeed, and the worst relative difference of the finite sums
        ok_same = bool(np.array_equal(sums[k][1], sums["off"][1]))
        m = sums["off"][1].astype(bool) & np.isfinite(sums["off"][0]) & (sums["off"][0] != 0)
        with np.errstate(all="ignore"):
            r["ok_equal_to_off"] = ok_same
            r["max_rel_diff_to_off"] = float(np.nanmax(np.abs(sums[k][0][m] - sums["off"][0][m]) / np.abs(sums["off"][0][m])))
    first_on = next(k for k in res if k != "off")
    rec = dict(label=args.label, nfeat=args.nfeat, ntrees=args.ntrees, rows=args.rows, dtype="f32", loss="L2",
               total_nodes=int(total_nodes), reps=args.reps, warmup=args.warmup, variants=res,
               on_median_below_off_min=bool(res[first_on]["kernel_ms_median"] < res["off"]["kernel_ms_min"]))
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    recs = json.loads(out.read_text()) if out.exists() else []
    recs.append(rec)
    out.write_text(json.dumps(recs, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
