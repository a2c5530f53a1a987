"""Expression operators as loss tree code (SRHIP_PROGRAM_EXPR_OP_TREE_CODE) against the same trees
interpreted, one process: 4096 random trees over {+, -, *, /, cos, exp} and the four non-lossy
operators of tests/expr_op_cases.py (custom_cos, op3, my_func_a, my_func_c) x 1M rows x 5 features,
Float32, L2 — the measurement population of DESIGN.md §3.13. Runs, alternated twice in this order:
the program without the flag (operator trees in the OPSET_EXPR interpreter: the yardstick), the
program with it; then once the expansions' plain tree code (the floor: the same arithmetic with
nothing opaque). Kernel ms per evaluation from srhip_last_kernel_time: median, min and max of
`steps` calls after `warmup`. A library without the keyword (an earlier build) measures the
unflagged program and the expansions only.
Writes profiles/expr_op_tree_code_timing.json.
Usage: python tools/bench_expr_op_tree_code.py [steps] [warmup] [output path]"""
import inspect
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "symbolicregression.jl_amd"), str(ROOT / "tests")]
import numpy as np  # noqa: E402


def main(steps=10, warmup=3, path=None):
    import expr_op_cases as E
    import srhip
    from srhip import constants as K

    T = np.float32
    o = E.options(E.NONLOSSY)
    trees = list(srhip.random_population(4096, o, 5, T, seed=0))
    flat = srhip.flatten(trees, o, dtype=T)
    xflat = srhip.flatten([E.expand(t, o) for t in trees], E.prim_options(), dtype=T)
    is_op = (flat.kind >= K.NODE_UNARY) & (flat.arg >= K.EXPR_OP_BEGIN)
    hold = sum(bool(is_op[flat.node_off[t]:flat.node_off[t + 1]].any()) for t in range(flat.ntrees))
    X = np.random.default_rng(1).standard_normal((5, 1_000_000)).astype(T)
    y = (T(2) * np.cos(X[3]) + X[0] * X[0] - T(2)).astype(T)
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, X, y)
    has_flag = "expr_op_tree_code" in inspect.signature(srhip.Program.__init__).parameters
    progs = {"flag off": srhip.Program(ctx, flat, T)}
    if has_flag:
        progs["flag on"] = srhip.Program(ctx, flat, T, expr_op_tree_code=True)
    order = list(progs) * 2 + ["expansions"]
    progs["expansions"] = srhip.Program(ctx, xflat, T)
    out = {"workload": "4096 trees over + - * / cos exp custom_cos op3 my_func_a my_func_c x 1M rows x 5 features, Float32, L2",
           "trees_holding_an_operator": hold, "nodes": int(flat.nodes.sum()), "expanded_nodes": int(xflat.nodes.sum()),
           "steps": steps, "warmup": warmup, "runs": []}
    for name in order:
        p = progs[name]
        ms = []
        for i in range(warmup + steps):
            s, w, ok = p.eval_loss(ds, K.LOSS["L2"])
            if i >= warmup:
                ms.append(ctx.last_kernel_time()[0])
        ok = np.asarray(ok).astype(bool)
        info = p.pass_info()
        run = {"run": name, "kernel_ms_median": float(np.median(ms)), "kernel_ms_min": min(ms), "kernel_ms_max": max(ms),
               "tree_code_trees": ctx.last_tree_code(), "shallow": info["shallow"], "deep": info["deep"],
               "kernel": ctx.last_kernel_name(), "ok": int(ok.sum()), "finite_sums": int(np.isfinite(s[ok]).sum())}
        out["runs"].append(run)
        print(run, flush=True)
    path = Path(path) if path else ROOT / "profiles" / "expr_op_tree_code_timing.json"
    path.parent.mkdir(exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    a = sys.argv[1:]
    main(int(a[0]) if a else 10, int(a[1]) if len(a) > 1 else 3, a[2] if len(a) > 2 else None)
