#!/usr/bin/env python3
"""Interleaved A/B of builds of the library and of per-launch knobs, in ONE process (GPU box).

The package is imported once per checkout (--root NAME=DIR; without one, this
checkout as "new"), under a name of its own (its imports are relative, and
each copy loads the libsrhip.so next to it), with a context, dataset and
program each. The variants' eval_loss calls then alternate A B C A B C ...,
so that clock drift and whatever else differs from process to process hits
all of them alike: process-per-variant A/Bs of the same build differ by
0.04-0.055 ms from process to process on config #2, several times the spread
inside one process. A variant is ROOT_NAME, ROOT_NAME:KEY=VALUE,KEY=VALUE or,
with one root, just KEY=VALUE,KEY=VALUE (knobs read per launch, set around
its calls; "" the defaults).

Per shape (--rows x --ntrees, comma lists; config #2's batch, seed 1000 as
bench.py, or a strided shard of it) and variant: the median kernel time (HIP
events) of each of --rounds rounds of --steps calls, their median and spread
(max − min), and whether loss sums and did_succeed equal the first variant's
bit for bit.

--loss NAME[:PARAM] (a comma list; default L2) times eval_loss with that elementwise loss, and --problem
jit_losses takes the batch of tests/test_jit_losses_gpu.py (1024 trees x 40 001 rows, --rows / --ntrees unused)
instead of config #2's: what a change to a loss routine is timed on.

Usage: python tools/ab_lib.py --root parent=/path/to/parent/checkout --root new=. [--rows 1000000,125000]
           [--ntrees 4096,512] [--rounds 5] [--steps 20] [--out FILE.json] parent new:SRHIP_JIT_TAIL_TREES=1 new
       python tools/ab_lib.py SRHIP_JIT_TAIL_TREES=1 SRHIP_JIT_TAIL_TREES=4,SRHIP_JIT_TAIL_ROUNDS=1.5
"""
import argparse
import importlib.util
import json
import os
import sys
from pathlib import Path


def load(name, root):
    pkg = Path(root).resolve() / "symbolicregression.jl_amd" / "srhip"
    spec = importlib.util.spec_from_file_location(name, pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class env:
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", action="append", help="NAME=checkout root (built); default new=this checkout")
    ap.add_argument("--rows", default="1000000")
    ap.add_argument("--ntrees", default="4096", help="4096, or strided shards of it (comma list)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loss", default="L2", help="NAME[:PARAM] of srhip.constants.LOSS, comma list")
    ap.add_argument("--problem", default="config2", choices=["config2", "jit_losses"])
    ap.add_argument("variants", nargs="+")
    args = ap.parse_args()
    import numpy as np

    os.environ.pop("SRHIP_LIB", None)  # each copy of the package loads the library of its own checkout
    roots = [r.split("=", 1) for r in (args.root or ["new=" + str(Path(__file__).resolve().parent.parent)])]
    mods = {name: load(f"srhip_ab{k}", root) for k, (name, root) in enumerate(roots)}
    vs = []
    for v in args.variants:
        name, sep, kv = v.partition(":")
        if name not in mods:  # knobs only: the (first) root
            name, kv = roots[0][0], v
        vs.append((v or "default", name, dict(x.split("=", 1) for x in kv.split(",") if x)))
    jl = args.problem == "jit_losses"
    rng = np.random.default_rng(71 if jl else 1)
    X = rng.standard_normal((5, 40_001 if jl else 1_000_000)).astype(np.float32)
    y = (np.float32(2) * np.cos(X[3]) + X[0] * X[0] - np.float32(2)).astype(np.float32)
    results = []
    shapes = [(1024, 40_001)] if jl else [(int(n), int(r)) for n in args.ntrees.split(",") for r in args.rows.split(",")]
    for lname, _, lpar in (l.partition(":") for l in args.loss.split(",")):
        for ntrees, rows in shapes:
            builds = {}
            for name, m in mods.items():
                o = m.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
                if jl:
                    trees = m.random_population(1024, o, 5, np.float32, seed=72)
                else:
                    trees = m.random_population(4096, o, 5, np.float32, seed=1000, maxsize=30)[:: 4096 // ntrees]
                ctx = m.get_context(0)
                ds = m.DeviceDataset(ctx, np.ascontiguousarray(X[:, :rows]), np.ascontiguousarray(y[:rows]))
                builds[name] = (ctx, ds, m.Program(ctx, m.flatten(trees, o, dtype=np.float32), np.float32),
                                (m.constants.LOSS[lname], [float(lpar)] if lpar else None))
            first, same = None, []
            for v, name, kv in vs:  # warm-up and the results
                ctx, ds, prog, L2 = builds[name]
                with env(kv):
                    for _ in range(5):
                        s, _, ok = prog.eval_loss(ds, *L2)
                got = (np.array(s, copy=True), np.array(ok, copy=True))
                first = first or got
                same.append(bool(np.array_equal(got[0], first[0], equal_nan=True) and np.array_equal(got[1], first[1])))
            med = [[] for _ in vs]
            for _ in range(args.rounds):
                ts = [[] for _ in vs]
                for _ in range(args.steps):
                    for k, (v, name, kv) in enumerate(vs):
                        ctx, ds, prog, L2 = builds[name]
                        with env(kv):
                            prog.eval_loss(ds, *L2)
                        ts[k].append(ctx.last_kernel_time()[0])
                for k in range(len(vs)):
                    med[k].append(float(np.median(ts[k])))
            for k, (v, name, kv) in enumerate(vs):
                r = dict(variant=v, loss=lname + (":" + lpar if lpar else ""), trees=ntrees, rows=rows, round_ms=[round(x, 5) for x in med[k]],
                         median_ms=round(float(np.median(med[k])), 5), spread_ms=round(max(med[k]) - min(med[k]), 5),
                         bit_identical_to_first=same[k], kernel=builds[name][0].last_kernel_name())
                results.append(r)
                print(json.dumps(r), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
