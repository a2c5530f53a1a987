#!/usr/bin/env python3
"""Timing of multi-output scoring: K targets over one X.

  case 1  Float32, L2, 5 features, 100k rows, K = 4, 66 trees per target (the launch
          size of search config #4): one step = the candidates of all four outputs.
            a  four srhip_eval_loss_batch_ctx calls on four plain datasets
            b  the same four calls on four views of one multi-target dataset
            c  one srhip_eval_loss_batch_targets_ctx call
  case 2  the same with 1024 trees per target and 1M rows: b (tree code) against c
          (interpreter); fixes the wrappers' switch between the two.
  case 3  device memory of K = 4 at 1M rows: four plain datasets against one
          multi-target dataset (hipMemGetInfo before / after the uploads).

Per leg: 3 warm-up steps, then 7 timed steps; wall time per step (perf_counter around the
calls, which return after their stream is drained) and the summed srhip_last_kernel_time.
Leg a uses entry points the parent commit has: --package / SRHIP_LIB point the tool at
another build's Python package and library, --legs a runs that leg alone there.

  python tools/bench_targets.py --case 1 --legs abc --tag new --out /tmp/tt/run1_new.json
  python tools/bench_targets.py --merge /tmp/tt/run*.json --out profiles/targets_timing.json
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
L2 = 0
K_TARGETS = 4
WARMUP, STEPS = 3, 7


def load_package(path):
    sys.path.insert(0, str(path))
    import srhip

    return srhip


def make_problem(srhip, n, per_target):
    o = srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
    rng = np.random.default_rng(7)
    X = rng.standard_normal((5, n)).astype(np.float32)
    Y = np.stack([(2 * np.cos(X[3]) + X[0] * X[0] - 2) * (1 + 0.25 * k) + 0.1 * k * X[k % 5]
                  for k in range(K_TARGETS)]).astype(np.float32)
    groups = [srhip.random_population(per_target, o, 5, np.float32, seed=100 + k) for k in range(K_TARGETS)]
    return o, X, Y, groups


def trees_struct(srhip, flat):
    from srhip._lib import Trees

    consts = np.ascontiguousarray(flat.consts, dtype=np.float32)
    keep = (flat.node_off, flat.kind, flat.arg, flat.const_off, consts)
    tr = Trees(flat.ntrees, flat.node_off.ctypes.data_as(C.POINTER(C.c_int32)),
               flat.kind.ctypes.data_as(C.POINTER(C.c_uint8)), flat.arg.ctypes.data_as(C.POINTER(C.c_uint16)),
               flat.const_off.ctypes.data_as(C.POINTER(C.c_int32)), consts.ctypes.data_as(C.c_void_p))
    return tr, keep


def time_leg(step, ctx):
    """step() runs one step and returns its summed kernel ms."""
    for _ in range(WARMUP):
        step()
    wall, kern = [], []
    for _ in range(STEPS):
        ctx.sync()
        t0 = time.perf_counter()
        k = step()
        wall.append((time.perf_counter() - t0) * 1e3)
        kern.append(k)
    return dict(wall_ms=wall, kernel_ms=kern, wall_ms_median=statistics.median(wall),
                kernel_ms_median=statistics.median(kern))


def run_case(srhip, case, legs):
    from srhip._lib import check, lib

    n, per = (100_000, 66) if case == 1 else (1_000_000, 1024)
    o, X, Y, groups = make_problem(srhip, n, per)
    ctx = srhip.get_context(0)
    L = lib()
    flats = [srhip.flatten(g, o, dtype=np.float32) for g in groups]
    structs = [trees_struct(srhip, f) for f in flats]
    allflat = srhip.flatten([t for g in groups for t in g], o, dtype=np.float32)
    allstruct = trees_struct(srhip, allflat)
    targets = np.repeat(np.arange(K_TARGETS), per).astype(np.int32)
    par = np.zeros(1)
    res = {}

    def per_target_step(handles):
        sums = np.empty(per)
        ok = np.empty(per, dtype=np.uint8)
        ws = C.c_double()

        def step():
            kms = 0.0
            for h, (tr, _) in zip(handles, structs):
                check(L.srhip_eval_loss_batch_ctx(ctx.handle, h, C.byref(tr), L2, par.ctypes.data, None, 0,
                                                  sums.ctypes.data, C.byref(ws), ok.ctypes.data))
                kms += ctx.last_kernel_time()[0]
            return kms
        return step

    if "a" in legs:
        plain = [srhip.DeviceDataset(ctx, X, Y[k]) for k in range(K_TARGETS)]
        res["a_plain_datasets"] = time_leg(per_target_step([d.handle for d in plain]), ctx)
        res["a_plain_datasets"]["tree_code_trees_last_call"] = ctx.last_tree_code()
        del plain
    if "b" in legs or "c" in legs:
        multi = srhip.MultiDeviceDataset(ctx, X, Y)
    if "b" in legs:
        views = [multi.view(k) for k in range(K_TARGETS)]
        res["b_views"] = time_leg(per_target_step([v.handle for v in views]), ctx)
        res["b_views"]["tree_code_trees_last_call"] = ctx.last_tree_code()
        vs, vok = [], []  # the views' results, for the check against the fused call
        for v, (tr, _) in zip(views, structs):
            s1, k1, w1 = np.empty(per), np.empty(per, dtype=np.uint8), C.c_double()
            check(L.srhip_eval_loss_batch_ctx(ctx.handle, v.handle, C.byref(tr), L2, par.ctypes.data, None, 0,
                                              s1.ctypes.data, C.byref(w1), k1.ctypes.data))
            vs.append(s1), vok.append(k1)
    if "c" in legs:
        nt = per * K_TARGETS
        sums = np.empty(nt)
        ok = np.empty(nt, dtype=np.uint8)
        ws = np.empty(K_TARGETS)

        def fused():
            check(L.srhip_eval_loss_batch_targets_ctx(ctx.handle, multi.handle, C.byref(allstruct[0]), L2,
                                                      par.ctypes.data, targets.ctypes.data, sums.ctypes.data,
                                                      ws.ctypes.data, ok.ctypes.data))
            return ctx.last_kernel_time()[0]
        res["c_fused"] = time_leg(fused, ctx)
        res["c_fused"]["kernel"] = ctx.last_kernel_name()
        if "b" in legs:  # both paths score the same trees on the same columns
            s0, k0 = np.concatenate(vs), np.concatenate(vok)
            fin = (k0 == 1) & np.isfinite(s0) & (s0 != 0)
            with np.errstate(all="ignore"):
                rel = np.abs(sums[fin] - s0[fin]) / np.abs(s0[fin])
            res["views_vs_fused"] = dict(ok_equal=bool(np.array_equal(k0, ok)), trees_ok=int((k0 == 1).sum()),
                                         compared=int(fin.sum()), max_rel_sum_difference=float(rel.max()),
                                         above_1e5=int((rel > 1e-5).sum()))
    return dict(rows=n, trees_per_target=per, targets=K_TARGETS, legs=res)


def run_memory(srhip):
    hip = C.CDLL("libamdhip64.so")

    def free_bytes():
        f, t = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    n = 1_000_000
    o, X, Y, _ = make_problem(srhip, n, 1)
    ctx = srhip.get_context(0)
    warm = srhip.DeviceDataset(ctx, X[:, :1000], Y[0, :1000])  # the runtime's own first allocations
    del warm
    ctx.sync()
    f0 = free_bytes()
    plain = [srhip.DeviceDataset(ctx, X, Y[k]) for k in range(K_TARGETS)]
    f1 = free_bytes()
    del plain
    ctx.sync()
    f2 = free_bytes()
    multi = srhip.MultiDeviceDataset(ctx, X, Y)
    views = [multi.view(k) for k in range(K_TARGETS)]
    f3 = free_bytes()
    n_pad = -(-n // 8192) * 8192
    return dict(rows=n, nfeat=5, targets=K_TARGETS, dtype="float32",
                four_plain_datasets_bytes=f0 - f1, one_multi_dataset_with_views_bytes=f2 - f3,
                expected_plain_bytes=K_TARGETS * (5 + 1) * n_pad * 4, expected_multi_bytes=(5 + K_TARGETS) * n_pad * 4,
                nviews=len(views))


def merge(files, out):
    runs = [json.loads(Path(f).read_text()) for f in sorted(files)]
    doc = dict(what="tools/bench_targets.py: multi-output scoring, the parent commit's build (leg a only) and this "
                    "build alternated in one session on one MI355X; per run 3 warm-up steps, 7 timed steps",
               unit="ms per step (one step = the candidates of all 4 targets)", runs=runs)
    for case in ("case1", "case2"):
        med = {}
        for r in runs:
            if case not in r:
                continue
            for leg, v in r[case]["legs"].items():
                if "wall_ms_median" not in v:  # (the views-against-fused record)
                    continue
                med.setdefault(f"{r['tag']}:{leg}", []).append(v["wall_ms_median"])
        if med:
            doc[case + "_wall_ms_medians"] = med
    pa = doc.get("case1_wall_ms_medians", {}).get("parent:a_plain_datasets")
    fc = doc.get("case1_wall_ms_medians", {}).get("new:c_fused")
    if pa and fc:
        doc["case1_verdict"] = dict(parent_a_fastest_run=min(pa), parent_a_range=[min(pa), max(pa)],
                                    fused_median_of_runs=statistics.median(fc),
                                    fused_is_a_gain=statistics.median(fc) < min(pa))
    Path(out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "runs"}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="1", help="1, 2, 3 or a list like 1,3")
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--tag", default="new")
    ap.add_argument("--package", default=str(ROOT / "symbolicregression.jl_amd"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--merge", nargs="+")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    srhip = load_package(a.package)
    doc = dict(tag=a.tag)
    for c in a.case.split(","):
        if c in ("1", "2"):
            doc["case" + c] = run_case(srhip, int(c), a.legs)
        elif c == "3":
            doc["case3"] = run_memory(srhip)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc)[:2000])


if __name__ == "__main__":
    main()
