"""Timing record of the derivative tree code against the forward-mode
interpreter of the same build: srhip_eval_loss_deriv on §3.18's shape, 4096 random trees x
1M rows x 5 features, Float32, L2, ndir = 1, 2 and 4, as kernel milliseconds
(srhip_last_kernel_time: the device events around the call's main kernels, the interpreter
kernel of the trees the generator refused included). The two programs — one made with
deriv_tree_code, one without — are called in turn in one process, `--warmup` times each
first; median, minimum and maximum of `--steps` calls each. The results of the two paths are
compared on the spot (flags equal; at least 99.9 % of the channel sums finite in both within
rtol of the interpreter's, the rest being trees whose derivative reaches 1e14 next to a pole,
where both paths are far from the Float64 value) so that a time is never recorded for a path
that computes something else.
The device has to be there; there is no fallback. Writes one JSON document.

Usage: bench_deriv_tree_code.py [--trees 4096] [--rows 1000000] [--steps 10] [--warmup 3]
                                [--out profiles/deriv_tree_code_timing.json]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "symbolicregression.jl_amd"))
import srhip  # noqa: E402
from srhip import constants as K  # noqa: E402
from srhip.engine import MultiDeviceDataset, Program  # noqa: E402

sys.path.insert(0, str(ROOT / "tools"))
from bench_deriv_loss import NFEAT, problem  # noqa: E402

DIRS = {1: [1], 2: [1, 4], 4: [1, 2, 4, 5]}


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rtol", type=float, default=1e-3, help="agreement of the two paths' channel sums")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "deriv_tree_code_timing.json"))
    args = ap.parse_args()
    if srhip.device_count() == 0:
        raise SystemExit("bench_deriv_tree_code: no HIP device")
    T = np.float32
    ctx = srhip.get_context(0)
    o, trees, X, y, G = problem(args.trees, args.rows)
    flat = srhip.flatten(trees, o, dtype=T)
    progs = dict(interpreter=Program(ctx, flat, T, interpreted=True),
                 tree_code=Program(ctx, flat, T, interpreted=True, deriv_tree_code=True))
    cases = []
    for ndir, dirs in DIRS.items():
        mds = MultiDeviceDataset(ctx, X, np.concatenate([y[None, :], G[[d - 1 for d in dirs]]]))
        d0 = [d - 1 for d in dirs]
        ms = {k: [] for k in progs}
        info, res = {}, {}
        for step in range(args.warmup + args.steps):
            for k, p in progs.items():  # alternated: both paths see the same machine
                res[k] = p.eval_loss_deriv(mds, K.LOSS["L2"], d0)
                if step >= args.warmup:
                    ms[k].append(ctx.last_kernel_time()[0])
                info[k] = dict(kernel=ctx.last_kernel_name(), launch=ctx.last_loss_launch(), compiled=ctx.last_tree_code())
        (si, _, oki), (st, _, okt) = res["interpreter"], res["tree_code"]
        both = oki & okt & np.isfinite(si).all(axis=1) & np.isfinite(st).all(axis=1)
        rel = np.abs(st[both] - si[both]) / np.maximum(np.abs(si[both]), 1e-30)
        worst = float(rel.max()) if both.any() else 0.0
        within = float((rel <= args.rtol).mean()) if both.any() else 1.0
        rec = dict(ndir=ndir, directions=dirs, flags_equal=bool(np.array_equal(oki, okt)), ok=int(okt.sum()),
                   finite_in_both=int(both.sum()), channels_within_rtol=within, worst_relative_difference=worst)
        for k in progs:
            rec[k] = dict(stats(ms[k]), **info[k])
        rec["tree_code"]["fallback_trees"] = args.trees - info["tree_code"]["compiled"]
        rec["ratio_interpreter_over_tree_code"] = rec["interpreter"]["median_ms"] / rec["tree_code"]["median_ms"]
        rec["below_interpreter_range"] = rec["tree_code"]["median_ms"] < rec["interpreter"]["min_ms"]
        cases.append(rec)
        print(json.dumps(rec))
        sys.stdout.flush()
        del mds
        if not rec["flags_equal"] or within < 0.999:
            raise SystemExit(f"bench_deriv_tree_code: the two paths disagree at ndir = {ndir} ({within:.4f} within rtol)")
    tc = {c["ndir"]: c["tree_code"]["median_ms"] for c in cases}
    doc = dict(tool="bench_deriv_tree_code", dtype="float32", loss="L2", nfeat=NFEAT, trees=args.trees, rows=args.rows,
               steps=args.steps, warmup=args.warmup, kernel_ms_source="srhip_last_kernel_time (device events)",
               order="interpreter, tree code, alternated per step in one process", cases=cases,
               tree_code_ndir4_over_ndir1=tc[max(tc)] / tc[min(tc)])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
