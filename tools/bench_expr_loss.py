"""Expression losses against their built-in counterparts on config #2's workload
(4096 trees x 1M rows, Float32), everything interpreted (SRHIP_JIT=0, so both
sides run eval_kernel): square(p - t) against L2DistLoss, and abs(p - t) ^ 2.5
against LPDistLoss(2.5). The expression side runs the loss program in the tile
epilogue (kModeLossExpr, 4 waves per SIMD for the shallow Float32 variant), the
built-in side a compiled epilogue (5 waves per SIMD).
Writes profiles/expr_loss_timing.json (kernel ms per evaluation: min and median
of `steps` calls after `warmup`, and the expression / built-in ratios).
Usage: python tools/bench_expr_loss.py [steps] [warmup] [output path]"""
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "symbolicregression.jl_amd")]
os.environ["SRHIP_JIT"] = "0"
import numpy as np  # noqa: E402


def main(steps=10, warmup=3, path=None):
    import srhip
    from srhip import Node

    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    lo = srhip.Options(binary_operators=["-", "^"], unary_operators=["square", "abs"])
    r = lo.make_binary("-", Node("x1"), Node("x2"))
    sq = srhip.ExprLoss(lo.make_unary("square", r), lo)
    e1 = srhip.ExprLoss(lo.make_binary("^", lo.make_unary("abs", r), Node(val=2.5)), lo)
    trees = srhip.random_population(4096, o, 5, np.float32, seed=0)
    X = np.random.default_rng(1).standard_normal((5, 1_000_000)).astype(np.float32)
    y = (np.float32(2) * np.cos(X[3]) + X[0] * X[0] - np.float32(2)).astype(np.float32)
    ctx = srhip.get_context(0)
    prog = srhip.Program(ctx, srhip.flatten(trees, o, dtype=np.float32), np.float32)
    ds = srhip.DeviceDataset(ctx, X, y)
    out = {"workload": "4096 trees x 1M rows, Float32, + - * / cos exp, SRHIP_JIT=0", "steps": steps,
           "warmup": warmup}
    for name, loss in (("L2DistLoss", srhip.L2DistLoss()), ("expr square(p - t)", sq),
                       ("LPDistLoss(2.5)", srhip.LPDistLoss(2.5)), ("expr abs(p - t) ^ 2.5", e1)):
        ms = []
        for i in range(warmup + steps):
            s, w, ok = prog.eval_loss(ds, loss.kind, loss.params)
            if i >= warmup:
                ms.append(ctx.last_kernel_time()[0])
        ok = np.asarray(ok).astype(bool)
        out[name] = {"kernel_ms_min": min(ms), "kernel_ms_median": float(np.median(ms)),
                     "tree_code_trees": ctx.last_tree_code(), "ok": int(ok.sum()),
                     "finite_sums": int(np.isfinite(s[ok]).sum())}
        print(name, out[name], flush=True)
    out["ratio_square_over_L2_median"] = out["expr square(p - t)"]["kernel_ms_median"] / out["L2DistLoss"]["kernel_ms_median"]
    out["ratio_pow_over_LP_median"] = out["expr abs(p - t) ^ 2.5"]["kernel_ms_median"] / out["LPDistLoss(2.5)"]["kernel_ms_median"]
    print("ratios", out["ratio_square_over_L2_median"], out["ratio_pow_over_LP_median"])
    path = Path(path) if path else ROOT / "profiles" / "expr_loss_timing.json"
    path.parent.mkdir(exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 10, int(a[1]) if len(a) > 1 else 3, a[2] if len(a) > 2 else None)
