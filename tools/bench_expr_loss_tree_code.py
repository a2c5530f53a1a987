"""Expression losses as loss tree code against their interpreted form and against L2, on config #2's
workload (4096 trees x 1M rows x 5 features, Float32, + - * / cos exp), one process:
square(p - t) and abs(p - t) ^ 2.5 through a handle made with tree_code=True (tree code, the
expression at the end of every tile) and through a plain handle (the whole call in the interpreter's
expression-loss mode), L2DistLoss as tree code and L2DistLoss interpreted (a program built with
SRHIP_JIT=0). A library without the tree_code keyword (an earlier build) measures the plain handles
and L2 only, so the same script gives the yardstick.
Writes profiles/expr_loss_tree_code_timing.json (kernel ms per evaluation from
srhip_last_kernel_time: median, min and max of `steps` calls after `warmup`).
Usage: python tools/bench_expr_loss_tree_code.py [steps] [warmup] [output path]"""
import inspect
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "symbolicregression.jl_amd")]
import numpy as np  # noqa: E402


def main(steps=10, warmup=3, path=None):
    import srhip
    from srhip import Node

    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    lo = srhip.Options(binary_operators=["-", "^"], unary_operators=["square", "abs"])
    r = lo.make_binary("-", Node("x1"), Node("x2"))
    exprs = {"SQ": lo.make_unary("square", r), "E1": lo.make_binary("^", lo.make_unary("abs", r), Node(val=2.5))}
    flat = srhip.flatten(srhip.random_population(4096, o, 5, np.float32, seed=0), o, dtype=np.float32)
    X = np.random.default_rng(1).standard_normal((5, 1_000_000)).astype(np.float32)
    y = (np.float32(2) * np.cos(X[3]) + X[0] * X[0] - np.float32(2)).astype(np.float32)
    ctx = srhip.get_context(0)
    prog = srhip.Program(ctx, flat, np.float32)
    os.environ["SRHIP_JIT"] = "0"
    interp = srhip.Program(ctx, flat, np.float32)
    del os.environ["SRHIP_JIT"]
    ds = srhip.DeviceDataset(ctx, X, y)
    flagged = "tree_code" in inspect.signature(srhip.ExprLoss.__init__).parameters
    runs = []
    for name, tree in exprs.items():
        if flagged:
            runs.append((f"{name} tree code", prog, srhip.ExprLoss(tree, lo, tree_code=True)))
        runs.append((f"{name} interpreted", prog, srhip.ExprLoss(tree, lo)))
    runs += [("L2DistLoss tree code", prog, srhip.L2DistLoss()), ("L2DistLoss interpreted", interp, srhip.L2DistLoss())]
    out = {"workload": "4096 trees x 1M rows x 5 features, Float32, + - * / cos exp", "steps": steps, "warmup": warmup}
    for name, p, loss in runs:
        ms = []
        for i in range(warmup + steps):
            s, w, ok = p.eval_loss(ds, loss.kind, loss.params)
            if i >= warmup:
                ms.append(ctx.last_kernel_time()[0])
        ok = np.asarray(ok).astype(bool)
        out[name] = {"kernel_ms_median": float(np.median(ms)), "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
                     "tree_code_trees": ctx.last_tree_code(), "kernel": ctx.last_kernel_name(), "ok": int(ok.sum()),
                     "finite_sums": int(np.isfinite(s[ok]).sum())}
        print(name, out[name], flush=True)
    path = Path(path) if path else ROOT / "profiles" / "expr_loss_tree_code_timing.json"
    path.parent.mkdir(exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 10, int(a[1]) if len(a) > 1 else 3, a[2] if len(a) > 2 else None)
