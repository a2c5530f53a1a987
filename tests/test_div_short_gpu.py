"""The packed divisions stop after one residual step (csrc/gen_jit.py manual_div,
manual_div_lc and their FAST forms: rcp, e = 1 - b*r, y = r + e*r, q = a*y,
s = a - b*q, q + s*y). That value is the IEEE quotient only if y = RN(1/b),
which rests on this hardware's v_rcp_f32 (tools/div_short_sweep.hip,
profiles/div_short_exhaustive.json: all 2^46 significand pairs, no mismatch).
Pinned here through the bodies themselves, as tree code:

  * x0 / x1 with x1 over ALL 2^23 significands against a few fixed numerators,
    and with x0 over all 2^23 significands against the divisors of
    tests/golden/div_short_divisors.json (the all-ones significand and the
    divisors at which tools/check_div_short.c finds the sequence intolerant of
    a reciprocal one ulp off), in the FAST region, the PRECISE region and as
    memory-constant code; once more near the FAST bound (|a| ~ 2^-49,
    |b| ~ 2^49);
  * c / x0 with x0 over all 2^23 significands for three constants;
  * a random population on mixed magnitudes against the compiled routines
    (SRHIP_JIT_MANUAL=0).

The tree is (quotient) - x_k with x_k numpy's Float32 quotient, y = 0: the L2
sum is exactly 0 iff every row's quotient equals numpy's bit for bit. Every
operand lies inside the packed range of the region under test, so no tile
leaves for the compiled routine, and no tile may be redone.
"""
import json
import os
from pathlib import Path

import numpy as np
import pytest

import srhip
from srhip import constants as K

pytestmark = pytest.mark.gpu

F32 = np.float32
NSIG = 1 << 23
CFG2 = dict(binary_operators=["+", "-", "*", "/"], unary_operators=["cos", "exp"])
GOLDEN = Path(__file__).resolve().parent / "golden" / "div_short_divisors.json"
# (SRHIP_JIT_FAST, memory-constant code)
MODES = {"fast": ("1", False), "precise": ("0", False), "memc": ("1", True)}


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def f32_hex(s):
    return F32(float.fromhex(s))


def all_significands(exponent=0):
    """Every Float32 of [2^e, 2^(e+1)), in order."""
    return ((np.arange(NSIG, dtype=np.uint32) | np.uint32(0x3f800000)).view(F32) * F32(2.0 ** exponent)).astype(F32)


def run(trees, o, ds, fast, memc=False, **kv):
    ctx = srhip.get_context(0)
    flat = srhip.flatten(trees, o, dtype=np.float32)
    with env(SRHIP_JIT="1", SRHIP_JIT_FAST=fast, **kv):
        prog = srhip.Program(ctx, flat, np.float32, varying_constants=memc)
        sums, _, ok = prog.eval_loss(ds, K.LOSS["L2"])
        info = prog.jit_info()
        bailed, redone = ctx.last_jit_events()
    return np.array(sums, copy=True), np.array(ok, copy=True), info, bailed, redone


def check_exact(trees, o, ds, mode, what):
    fast, memc = MODES[mode]
    s, ok, info, bailed, redone = run(trees, o, ds, fast, memc)
    print(f"{what}, {mode}: {info['ntrees']} trees as tree code, {info['nfast']} FAST, {bailed} handed back, "
          f"{redone} tiles redone, sums {s}")
    assert info["ntrees"] == len(trees)
    assert info["nfast"] == (len(trees) if fast == "1" else 0)
    assert bailed == 0 and redone == 0  # every tile ran the region's packed body to the end
    assert ok.all(), np.flatnonzero(~ok)
    assert np.all(s == 0), (np.flatnonzero(s != 0), s[s != 0])


def var_div_problem(cols, pairs):
    """Features: the columns, then cols[i] / cols[j] per pair (i, j); the trees
    (x_i / x_j) - q_ij. Each quotient stands in one tree only, so none becomes
    a shared column."""
    with np.errstate(all="raise"):
        X = np.stack(list(cols) + [cols[i] / cols[j] for i, j in pairs]).astype(F32)
    assert np.isfinite(X).all() and X.shape[1] % 256 == 0
    o = srhip.Options(**CFG2)
    N = srhip.Node
    trees = [o.make_binary("-", o.make_binary("/", N(feature=1 + i), N(feature=1 + j)), N(feature=1 + len(cols) + k))
             for k, (i, j) in enumerate(pairs)]
    ds = srhip.DeviceDataset(srhip.get_context(0), X, np.zeros(X.shape[1], F32))
    return o, trees, ds


NUMERATORS = ["0x1.fffffep0", "0x1.000002p0", "0x1p0", "-0x1.555556p0"]


@pytest.fixture(scope="module")
def every_divisor(gpu_ctx):
    n = len(NUMERATORS)
    return var_div_problem([np.full(NSIG, f32_hex(h)) for h in NUMERATORS] + [all_significands()],
                           [(j, n) for j in range(n)])


@pytest.mark.parametrize("mode", list(MODES))
def test_every_divisor_significand(every_divisor, mode):
    o, trees, ds = every_divisor
    check_exact(trees, o, ds, mode, "x1 over all significands")


def golden_divisors():
    g = json.loads(GOLDEN.read_text())
    d = [int(h, 16) for h in g["divisors"]]
    assert 0x3fffffff in d and 1 <= len(d) <= 8  # the all-ones significand, whatever the sweep's set holds
    return d


# four divisors per dataset (9 columns of 2^23 rows)
@pytest.fixture(scope="module", params=range((len(golden_divisors()) + 3) // 4))
def every_numerator(gpu_ctx, request):
    d = golden_divisors()[4 * request.param:4 * request.param + 4]
    return var_div_problem([all_significands()] + [np.full(NSIG, np.uint32(u).view(F32)) for u in d],
                           [(0, 1 + j) for j in range(len(d))])


@pytest.mark.parametrize("mode", list(MODES))
def test_every_numerator_significand_at_the_exception_divisors(every_numerator, mode):
    o, trees, ds = every_numerator
    check_exact(trees, o, ds, mode, "x0 over all significands")


def test_every_divisor_significand_near_the_fast_bound(gpu_ctx):
    """|a| ~ 2^-49 and |b| ~ 2^49: inside the FAST bodies' lower bound
    (min(|a|, |rcp(b)|) >= 2^-50), quotients ~ 2^-98. The PRECISE bodies send
    such a tile to the compiled routine, so only the FAST region is run."""
    o, trees, ds = var_div_problem([np.full(NSIG, f32_hex("0x1.fffffep-49")), np.full(NSIG, f32_hex("-0x1.000002p-49")),
                                    all_significands(49)], [(0, 2), (1, 2)])
    check_exact(trees, o, ds, "fast", "near the FAST bound")


@pytest.fixture(scope="module")
def constant_numerator(gpu_ctx):
    c = [f32_hex("0x1.fffffep0"), f32_hex("0x1.000002p3"), F32(-3.0)]
    b = all_significands()
    X = np.stack([b] + [cj / b for cj in c]).astype(F32)
    assert np.isfinite(X).all()
    o = srhip.Options(**CFG2)
    N = srhip.Node
    trees = [o.make_binary("-", o.make_binary("/", N(val=cj), N(feature=1)), N(feature=2 + j)) for j, cj in enumerate(c)]
    return o, trees, srhip.DeviceDataset(gpu_ctx, X, np.zeros(NSIG, F32))


@pytest.mark.parametrize("mode", list(MODES))
def test_constant_numerator_every_divisor_significand(constant_numerator, mode):
    o, trees, ds = constant_numerator
    check_exact(trees, o, ds, mode, "c / x0")


def test_random_population_equals_compiled_routines(gpu_ctx):
    """As tests/test_jit_gpu.py's comparison: did_succeed and sums of the
    hand-scheduled bodies equal those of hipcc's routines, both regions."""
    o = srhip.Options(**CFG2)
    trees = srhip.random_population(300, o, 5, np.float32, seed=141)
    rng = np.random.default_rng(142)
    n = 20_480
    X = (rng.standard_normal((5, n)) * rng.choice([1e-3, 1.0, 30.0, 1e4], (5, n))).astype(F32)
    X[:, :256] = rng.uniform(0.5, 2.0, (5, 256)).astype(F32)  # one tile with every division in range
    y = (F32(2) * np.cos(X[3]) + X[0] * X[0] - F32(2)).astype(F32)
    ds = srhip.DeviceDataset(gpu_ctx, X, y)
    for fast in ("1", "0"):
        s_m, ok_m, info_m, _, redone = run(trees, o, ds, fast)
        s_f, ok_f, info_f, _, _ = run(trees, o, ds, fast, SRHIP_JIT_MANUAL="0")
        print(f"fast={fast}: {info_m['ntrees']} trees, {info_m['nfast']} FAST, {redone} tiles redone, "
              f"{int(ok_m.sum())} succeeded")
        assert info_m["ntrees"] == info_f["ntrees"] > 200
        assert np.array_equal(ok_m, ok_f)
        assert np.array_equal(s_m[ok_m], s_f[ok_f])
