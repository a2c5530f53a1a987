#!/usr/bin/env python3
"""Real use of the column pool (GPU box): one dataset, N populations from N
seeds, each population compiled and evaluated ONCE, as a search does — not
bench.py's one program evaluated over and over.

Per population: the time to create the program, the time of its one eval_loss
call (host clock around the synchronous call: the derive program's build and
code-object load, the derive pass and the tree code) and the call's kernel
time; then the context's counters (columns derived / reused, derive programs
built) where the library has them.

--root DIR     import srhip from DIR/symbolicregression.jl_amd (another checkout, to compare)
--fresh-dataset  a new dataset per population: every call finds an empty pool (the all-miss case)

Usage: python tools/bench_populations.py [--root DIR] [--rows 1000000] [--ntrees 4096] [--populations 20]
"""
import argparse
import json
import sys
import time
from pathlib import Path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--ntrees", type=int, default=4096)
    ap.add_argument("--populations", type=int, default=20)
    ap.add_argument("--fresh-dataset", action="store_true")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve() / "symbolicregression.jl_amd"))
    import numpy as np

    import srhip
    from srhip import constants as K

    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    rng = np.random.default_rng(1)
    X = rng.standard_normal((5, args.rows)).astype(np.float32)
    y = (np.float32(2) * np.cos(X[3]) + X[0] * X[0] - np.float32(2)).astype(np.float32)
    flats = [srhip.flatten(srhip.random_population(args.ntrees, o, 5, np.float32, seed=1000 + 37 * k, maxsize=30), o,
                           dtype=np.float32) for k in range(args.populations)]
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    warm = srhip.Program(ctx, srhip.flatten(srhip.random_population(256, o, 5, np.float32, seed=1, maxsize=30), o,
                                            dtype=np.float32), np.float32)
    warm.eval_loss(ds, K.LOSS["L2"])  # the library's own first-call costs, outside every population
    del warm
    info = getattr(ctx, "column_cache_info", None)
    base = info() if info else None
    create_ms, call_ms, kernel_ms, checks = [], [], [], []
    for flat in flats:
        if args.fresh_dataset:
            ds = srhip.DeviceDataset(ctx, X, y)
        t0 = time.perf_counter()
        p = srhip.Program(ctx, flat, np.float32)
        t1 = time.perf_counter()
        s, w, ok = p.eval_loss(ds, K.LOSS["L2"])
        t2 = time.perf_counter()
        create_ms.append((t1 - t0) * 1e3)
        call_ms.append((t2 - t1) * 1e3)
        kernel_ms.append(ctx.last_kernel_time()[0])
        checks.append([int(ok.sum()), float(np.sum(s[ok]))])
        del p
    out = dict(tool="bench_populations", tag=args.tag, rows=args.rows, ntrees=args.ntrees,
               populations=args.populations, fresh_dataset=args.fresh_dataset,
               create_ms=create_ms, call_ms=call_ms, kernel_ms=kernel_ms,
               call_ms_median=float(np.median(call_ms)), call_ms_first=call_ms[0],
               call_ms_median_after_first=float(np.median(call_ms[1:])) if len(call_ms) > 1 else None,
               kernel_ms_median=float(np.median(kernel_ms)), create_ms_median=float(np.median(create_ms)),
               checks=checks)
    if info:
        now = info()
        out["counters"] = {k: now[k] - base[k] for k in ("derived", "reused", "programs")}
        out["nslot"] = now["nslot"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
