"""Expression-loss gradients as gradient tree code against their interpreted form and against the L2
gradient tree code, on config #2's workload (4096 trees x 1M rows x 5 features, Float32, + - * / cos
exp), one srhip_eval_loss_grad call per sample, the variants alternated in one process:
square(p - t) and square(p - t) / (abs(t) + 1) through a handle made with grad_tree_code=True (the
expression's forward and reverse sweep inside every tile) and through a plain handle (grad_kernel's
forward-mode expression mode), and L2DistLoss on the same program. A library that refuses the flag
(an earlier build, through SRHIP_LIB) measures the plain handles and L2 only, so the same script
gives the yardstick.
Writes profiles/expr_loss_grad_timing.json (kernel ms per call from srhip_last_kernel_time: median,
min and max of `steps` calls after `warmup`; trees that ran as tree code; trees that fell back).
Usage: python tools/bench_expr_loss_grad.py [steps] [warmup] [output path]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "symbolicregression.jl_amd")]
import numpy as np  # noqa: E402


def main(steps=10, warmup=3, path=None):
    import srhip
    from srhip import Node

    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    lo = srhip.Options(binary_operators=["-", "+", "/"], unary_operators=["square", "abs"])
    sq = lo.make_unary("square", lo.make_binary("-", Node("x1"), Node("x2")))
    exprs = {"SQ": sq, "E2": lo.make_binary("/", sq.copy(), lo.make_binary("+", lo.make_unary("abs", Node("x2")), Node(val=1.0)))}
    flat = srhip.flatten(srhip.random_population(4096, o, 5, np.float32, seed=0), o, dtype=np.float32)
    X = np.random.default_rng(1).standard_normal((5, 1_000_000)).astype(np.float32)
    y = (np.float32(2) * np.cos(X[3]) + X[0] * X[0] - np.float32(2)).astype(np.float32)
    ctx = srhip.get_context(0)
    prog = srhip.Program(ctx, flat, np.float32)
    ds = srhip.DeviceDataset(ctx, X, y)
    runs = []
    for name, tree in exprs.items():
        try:  # a library from before the flag refuses it: the plain handles and L2 are the yardstick
            runs.append((f"{name} tree code", srhip.ExprLoss(tree, lo, grad_tree_code=True)))
        except (srhip.SrhipError, TypeError):
            pass
        runs.append((f"{name} interpreted", srhip.ExprLoss(tree, lo)))
    runs.append(("L2DistLoss tree code", srhip.L2DistLoss()))
    ms = {name: [] for name, _ in runs}
    last = {}
    for i in range(warmup + steps):  # alternated: every variant sees the same drift
        for name, loss in runs:
            s, g, w, ok = prog.eval_loss_grad(ds, loss.kind, loss.params)
            if i >= warmup:
                ms[name].append(ctx.last_kernel_time()[0])
            last[name] = (ctx.last_tree_code(), ctx.last_kernel_name(), int(np.asarray(ok).sum()))
    out = {"workload": "4096 trees x 1M rows x 5 features, Float32, + - * / cos exp; srhip_eval_loss_grad",
           "steps": steps, "warmup": warmup, "gradient_candidates": prog.grad_jit_info()}
    for name, _ in runs:
        ran, kernel, nok = last[name]
        out[name] = {"kernel_ms_median": float(np.median(ms[name])), "kernel_ms_min": min(ms[name]),
                     "kernel_ms_max": max(ms[name]), "tree_code_trees": ran, "interpreted_trees": flat.ntrees - ran,
                     "last_kernel": kernel, "ok": nok}
        print(name, out[name], flush=True)
    path = Path(path) if path else ROOT / "profiles" / "expr_loss_grad_timing.json"
    path.parent.mkdir(exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 10, int(a[1]) if len(a) > 1 else 3, a[2] if len(a) > 2 else None)
