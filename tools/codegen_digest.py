#!/usr/bin/env python3
"""Digest of the tree compilers' emitted machine code over a fixed corpus (no device).

    SRHIP_LIB=/path/to/libsrhip.so python tools/codegen_digest.py [--out digests.json]

prints {case: sha256(code bytes, tree offsets)}. Two libraries whose digests are all equal generate the
same code for the corpus, so a change to the generators (csrc/jit.cpp, jit_grad.cpp, jit64.cpp) that is
meant to leave the code alone is checked by running this once per library, with no SRHIP_* switch set,
and again under each code-generation switch the tests use (SRHIP_JIT_PACKED=0, SRHIP_JIT_PKMOV=0,
SRHIP_JIT_MANUAL=0, SRHIP_JIT_TRIG_FULL=1, SRHIP_JIT_TRIM_ROOT=0, SRHIP_GJIT_GCOLS=0).

Corpus: config #2's 4096 trees, config #5's trees, a batch with shared subtrees, a wide batch (96
features). Settings: Float32 loss code fast x memc, per-row output code, gradient code, every built-in
loss as tile tail (FAST and PRECISE) and as gradient seed in both dtypes, the Float64 loss, output and
gradient code, the wide loss code (L2 and each loss). A case whose compile is refused (a loss without
tree code in that dtype) is recorded as "error: ..." — equal between libraries like any other digest.
"""
import argparse
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "symbolicregression.jl_amd"))
import srhip  # noqa: E402
from srhip.engine import jit_compile  # noqa: E402

F32, F64 = np.float32, np.float64
CFG2 = (["+", "-", "*", "/"], ["cos", "exp"])
MIXED = (["+", "*", "/", "-", "^", "max", "min", "mod"], ["safe_log", "safe_sqrt", "tanh", "relu", "inv", "sign"])
TRIG = (["+", "-", "*", "/"], ["sin", "cos", "exp", "neg", "square", "cube", "abs"])
LOSSES = {
    "L1": srhip.L1DistLoss(), "LP2.5": srhip.LPDistLoss(2.5), "LPINT3": srhip.LPDistLoss(3),
    "Huber": srhip.HuberLoss(0.7), "LogCosh": srhip.LogCoshLoss(), "L1EpsIns": srhip.L1EpsilonInsLoss(0.3),
    "L2EpsIns": srhip.L2EpsilonInsLoss(0.25), "Quantile": srhip.QuantileLoss(0.8), "Periodic": srhip.PeriodicLoss(2.0),
    "LogitDist": srhip.LogitDistLoss(), "ZeroOne": srhip.ZeroOneLoss(), "Perceptron": srhip.PerceptronLoss(),
    "LogitMargin": srhip.LogitMarginLoss(), "L1Hinge": srhip.L1HingeLoss(), "L2Hinge": srhip.L2HingeLoss(),
    "SmoothedL1Hinge": srhip.SmoothedL1HingeLoss(0.5), "ModHuber": srhip.ModifiedHuberLoss(),
    "L2Margin": srhip.L2MarginLoss(), "Exp": srhip.ExpLoss(), "Sigmoid": srhip.SigmoidLoss(), "DWDMargin": srhip.DWDMarginLoss(2.0),
}


def flat_of(ops, n, nfeat, dtype, seed):
    o = srhip.Options(binary_operators=ops[0], unary_operators=ops[1])
    return srhip.flatten(srhip.random_population(n, o, nfeat, dtype, seed=seed), o, dtype=dtype)


def digest(flat, **kw):
    try:
        code, _, offs = jit_compile(flat, **kw)
    except Exception as e:  # a refused compile is part of the behaviour
        return f"error: {type(e).__name__}: {e}"[:200]
    h = hashlib.sha256(code)
    h.update(np.asarray(sorted(offs.items()), dtype=np.int64).tobytes())
    return h.hexdigest()


def corpus():
    out = {}
    big = {"cfg2": flat_of(CFG2, 4096, 5, F32, 0), "cfg5": flat_of(CFG2, 2000, 20, F32, 5),
           "shared": flat_of(CFG2, 1500, 5, F32, 1000), "mixed": flat_of(MIXED, 600, 7, F32, 13),
           "trig": flat_of(TRIG, 600, 7, F32, 12)}
    for name, flat in big.items():
        for fast in (0, 1):
            for memc in (0, 1):
                out[f"{name}/f32/loss/fast{fast}/memc{memc}"] = digest(flat, fast=bool(fast), memc=bool(memc))
        out[f"{name}/f32/out"] = digest(flat, out=True)
        out[f"{name}/f32/grad"] = digest(flat, grad=True)
    wide = flat_of(CFG2, 600, 96, F32, 7)
    for fast in (0, 1):
        out[f"wide96/f32/loss/fast{fast}"] = digest(wide, fast=bool(fast), wide=True)
        out[f"wide96/f32/loss/fast{fast}/notwide"] = digest(wide, fast=bool(fast))
    out["wide96/f32/grad"] = digest(wide, grad=True)
    big64 = {"cfg2": flat_of(CFG2, 1000, 5, F64, 0), "cfg5": flat_of(CFG2, 1000, 20, F64, 5),
             "cfg3": flat_of((["+", "-", "*", "/", "^"], ["safe_log", "safe_sqrt", "cos", "exp"]), 600, 7, F64, 53),
             "mixed": flat_of(MIXED, 600, 7, F64, 13)}
    for name, flat in big64.items():
        out[f"{name}/f64/loss"] = digest(flat)
        out[f"{name}/f64/out"] = digest(flat, out=True)
        out[f"{name}/f64/grad"] = digest(flat, grad=True)
    small = {"f32": flat_of(CFG2, 300, 5, F32, 31), "f64": flat_of(CFG2, 300, 5, F64, 61)}
    swide = flat_of(CFG2, 200, 96, F32, 8)
    for lname, loss in LOSSES.items():
        for fast in (0, 1):
            out[f"loss/{lname}/f32/tail/fast{fast}"] = digest(small["f32"], fast=bool(fast), loss=loss)
        out[f"loss/{lname}/f32/tail/wide"] = digest(swide, fast=True, loss=loss, wide=True)
        out[f"loss/{lname}/f32/seed"] = digest(small["f32"], grad=True, fast=False, loss=loss)
        out[f"loss/{lname}/f64/tail"] = digest(small["f64"], loss=loss)
        out[f"loss/{lname}/f64/seed"] = digest(small["f64"], grad=True, loss=loss)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", help="also write the JSON here")
    a = ap.parse_args()
    text = json.dumps(corpus(), indent=1, sort_keys=True)
    if a.out:
        Path(a.out).write_text(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
