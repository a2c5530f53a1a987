"""Loss tree code of a margin loss against its distance twin on config #2
(4096 trees x 1M rows, Float32): LogitMarginLoss and LogitDistLoss end each
tile with log1p(exp(.)) routines that differ by a multiply (ŷ·y) in place of
a subtract (ŷ - y) in front, so their times should agree; L2 is the baseline.
With y ∈ {-1, +1} for the margin loss, the regression y for the others.
Writes profiles/margin_loss_timing.json (kernel ms per evaluation: min and
median of `steps` calls after `warmup`).
Usage: python tools/bench_margin.py [steps] [warmup]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "symbolicregression.jl_amd")]
import numpy as np  # noqa: E402


def main(steps=20, warmup=5):
    import srhip

    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    trees = srhip.random_population(4096, o, 5, np.float32, seed=0)
    X = np.random.default_rng(1).standard_normal((5, 1_000_000)).astype(np.float32)
    yr = (np.float32(2) * np.cos(X[3]) + X[0] * X[0] - np.float32(2)).astype(np.float32)
    yc = np.where(yr >= 0, 1, -1).astype(np.float32)
    ctx = srhip.get_context(0)
    prog = srhip.Program(ctx, srhip.flatten(trees, o, dtype=np.float32), np.float32)
    out = {"workload": "4096 trees x 1M rows, Float32, + - * / cos exp", "steps": steps, "warmup": warmup}
    for name, loss, y in (("L2DistLoss", srhip.L2DistLoss(), yr), ("LogitDistLoss", srhip.LogitDistLoss(), yr),
                          ("LogitMarginLoss", srhip.LogitMarginLoss(), yc)):
        ds = srhip.DeviceDataset(ctx, X, y)
        ms = []
        for i in range(warmup + steps):
            s, w, ok = prog.eval_loss(ds, loss.kind, loss.params)
            if i >= warmup:
                ms.append(ctx.last_kernel_time()[0])
        out[name] = {"kernel_ms_min": min(ms), "kernel_ms_median": float(np.median(ms)),
                     "tree_code_trees": ctx.last_tree_code(), "jit_events": list(ctx.last_jit_events()),
                     "ok": int(np.asarray(ok).astype(bool).sum())}
        print(name, out[name], flush=True)
    out["ratio_margin_over_dist_median"] = out["LogitMarginLoss"]["kernel_ms_median"] / out["LogitDistLoss"]["kernel_ms_median"]
    print("ratio", out["ratio_margin_over_dist_median"])
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "margin_loss_timing.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
