"""Generate tests/golden/deriv_grad_cases.npz — per-row references for the constant gradients
of a derivative objective (run by hand on the CPU:
python tests/golden/make_deriv_grad_golden.py; needs mpmath 1.3; a few minutes on 16 processes).

Trees: 24 random ones over `+ - * / cos exp` and 4 features (seed fixed; the generator draws
on until it has 24 that keep value, derivative and mixed partial finite and below 1e6 on
every row, hold at least one constant, and of which at least six hold more constants than the
kernels' constant group, 2), and hand-made ones for safe_pow, sqrt, log and tanh. X is 293
standard normal rows rounded to Float32 and every constant is a Float32 value, so both
dtypes see the same operands and one set of reference values serves both.

Per tree, row, direction in DIRS and constant: ŷ, ∂ŷ/∂c, ∂ŷ/∂x and ∂²ŷ/∂x∂c from mpmath.diff
on the tree written as an mpmath function (30 digits; the differences' own error is far
below Float64's), and per dtype T their largest movement when every operand (features and
constants) is scaled by 1 + 4·eps(T) and by 1 − 4·eps(T). A movement is stored as the
exponent of the next power of two (uint16), which keeps the file within the size of the
largest fixture: the conditioning term a test takes from it is at most twice the movement.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "symbolicregression.jl_amd")]

NROWS = 293
DIRS = (1, 3)
NRANDOM = 24
GC = 2
LIMIT = 1e6
MAX_CONSTS = 4  # of a random tree: keeps the file small
BIAS = 1100
BIN = ["+", "-", "*", "/", "safe_pow"]
UNA = ["cos", "exp", "safe_sqrt", "safe_log", "tanh"]


def options():
    import srhip

    return srhip.Options(binary_operators=BIN, unary_operators=UNA)


def random_options():
    import srhip

    return srhip.Options(binary_operators=BIN[:4], unary_operators=UNA[:2])


def features():
    X = np.random.default_rng(301).standard_normal((4, NROWS))
    X[2] = np.abs(X[2]) + 0.5  # x3 > 0: the hand-made trees take its log, root and powers
    return X.astype(np.float32).astype(np.float64)


def hand_trees(o):
    from srhip import Node

    B, U = o.make_binary, o.make_unary
    c = lambda v: Node(val=float(np.float32(v)))
    return [B("*", c(1.25), B("safe_pow", B("+", Node("x3"), c(0.5)), c(1.5))),
            B("+", U("safe_sqrt", B("*", c(0.75), Node("x3"))), B("*", c(-0.5), Node("x1"))),
            B("*", c(2.0), U("safe_log", B("+", B("*", c(0.5), Node("x3")), B("*", Node("x1"), Node("x1"))))),
            U("tanh", B("+", B("*", c(0.5), Node("x1")), B("*", c(-0.25), B("*", Node("x3"), Node("x1")))))]


def candidates():
    """Random trees in drawing order (the oracle-free filters come later, in mpmath)."""
    import srhip

    o = random_options()
    seed = 0
    while True:
        for t in srhip.random_population(64, o, 4, np.float32, seed=400 + seed, maxsize=14):
            yield t
        seed += 1


def const_nodes(tree):
    from srhip.node import _postorder

    return [n for n in _postorder(tree) if n.degree == 0 and n.constant]


def as_function(tree, o, mp):
    """f(x1..x4, c1..cn) in mpmath; constants in the order of flatten (post-order)."""
    cn = const_nodes(tree)
    index = {id(n): k for k, n in enumerate(cn)}
    bn, un = list(o.binary_operators), list(o.unary_operators)

    def ev(n, xs, cs):
        if n.degree == 0:
            return cs[index[id(n)]] if n.constant else xs[n.feature - 1]
        if n.degree == 1:
            a = ev(n.l, xs, cs)
            name = un[n.op - 1]
            return {"cos": mp.cos, "exp": mp.exp, "safe_sqrt": mp.sqrt, "safe_log": mp.log, "tanh": mp.tanh}[name](a)
        a, b = ev(n.l, xs, cs), ev(n.r, xs, cs)
        name = bn[n.op - 1]
        if name == "+":
            return a + b
        if name == "-":
            return a - b
        if name == "*":
            return a * b
        if name == "/":
            return a / b
        return a ** b

    return (lambda *args: ev(tree, args[:4], args[4:])), [float(n.val) for n in cn]


def evaluate(tree, X):
    """(v [n], dc [nc, n], dx [ndir, n], dxc [nc, ndir, n]) and the movements per dtype, or None when a
    value is not finite or reaches LIMIT."""
    import mpmath as mp

    mp.mp.dps = 30
    o = options()
    f, cs = as_function(tree, o, mp)
    nc, n, nd = len(cs), X.shape[1], len(DIRS)

    def at(xs, cv):
        args = [mp.mpf(v) for v in xs] + [mp.mpf(v) for v in cv]
        v = f(*args)
        out = [v]
        for j in range(nc):
            od = [0] * len(args)
            od[4 + j] = 1
            out.append(mp.diff(f, tuple(args), tuple(od)))
        for d in DIRS:
            od = [0] * len(args)
            od[d - 1] = 1
            out.append(mp.diff(f, tuple(args), tuple(od)))
        for j in range(nc):
            for d in DIRS:
                od = [0] * len(args)
                od[d - 1] = 1
                od[4 + j] = 1
                out.append(mp.diff(f, tuple(args), tuple(od)))
        vals = []
        for q in out:
            if hasattr(q, "imag") and q.imag != 0:
                return None
            vals.append(float(mp.re(q)))
        return np.asarray(vals)

    nq = 1 + nc + nd + nc * nd
    base = np.zeros((nq, n))
    move = {tn: np.zeros((nq, n)) for tn in ("f32", "f64")}
    for i in range(n):
        try:
            b = at(X[:, i], cs)
        except (ValueError, ZeroDivisionError):
            return None
        if b is None or not np.isfinite(b).all() or np.abs(b).max() >= LIMIT:
            return None
        base[:, i] = b
        for tn, T in (("f32", np.float32), ("f64", np.float64)):
            e4 = 4 * float(np.finfo(T).eps)
            for s in (1 + e4, 1 - e4):
                try:
                    m = at(X[:, i] * s, [v * s for v in cs])
                except (ValueError, ZeroDivisionError):
                    m = None
                mv = np.full(nq, np.inf) if m is None else np.abs(m - b)
                move[tn][:, i] = np.maximum(move[tn][:, i], np.where(np.isnan(mv), np.inf, mv))
    return base, move


def _job(args):
    tree, X = args
    return evaluate(tree, X)


def trees():
    """The fixture's trees, as the stored selection (`picked`) names them among the candidates."""
    with np.load(Path(__file__).with_name("deriv_grad_cases.npz")) as z:
        picked = [int(k) for k in z["picked"]]
    return select(picked)


def select(picked):
    out, want = [], set(picked)
    for k, t in enumerate(candidates()):
        if k in want:
            out.append(t)
        if k >= max(picked):
            break
    return out + hand_trees(options())


def encode(m):
    """ceil(log2(movement)) + BIAS as uint16; 0 for no movement."""
    with np.errstate(divide="ignore"):
        e = np.ceil(np.log2(m))
    if not np.isfinite(m).all():
        raise SystemExit("a movement is not finite: no working bound")
    return np.where(m > 0, np.clip(e + BIAS, 1, 65535), 0).astype(np.uint16)


def decode(code):
    """The stored movement's upper bound (a power of two)."""
    c = np.asarray(code, dtype=np.float64)
    return np.where(c > 0, np.exp2(c - BIAS), 0.0)


def main():
    from multiprocessing import Pool

    X = features()
    results, picked, many = [], [], 0
    gen = enumerate(candidates())
    with Pool(16) as pool:
        while len(picked) < NRANDOM:
            batch = []
            while len(batch) < 32:
                k, t = next(gen)
                nc = len(const_nodes(t))
                if 1 <= nc <= MAX_CONSTS:
                    batch.append((k, t))
            for (k, t), r in zip(batch, pool.map(_job, [(t, X) for _, t in batch])):
                if r is None or len(picked) >= NRANDOM:
                    continue
                nc = len(const_nodes(t))
                # the last places go to trees with more constants than GC until six are in
                if nc <= GC and NRANDOM - len(picked) <= 6 - many:
                    continue
                many += nc > GC
                picked.append(k)
                results.append(r)
        hand = hand_trees(options())
        hr = pool.map(_job, [(t, X) for t in hand])
    for t, r in zip(hand, hr):
        if r is None:
            raise SystemExit(f"a hand-made tree leaves the limits: {t!r}")
        results.append(r)
    assert many >= 6
    all_trees = select(picked)
    ncs = [len(const_nodes(t)) for t in all_trees]
    coff = np.concatenate([[0], np.cumsum(ncs)]).astype(np.int32)
    nd, n = len(DIRS), NROWS
    out = {"picked": np.asarray(picked, dtype=np.int32), "ntrees": np.int32(len(all_trees)), "dirs": np.asarray(DIRS, dtype=np.int32),
           "const_off": coff, "X": X}
    v = np.zeros((len(all_trees), n))
    dx = np.zeros((len(all_trees), nd, n))
    dc = np.zeros((coff[-1], n))
    dxc = np.zeros((coff[-1], nd, n))
    sp = {tn: [np.zeros_like(v), np.zeros_like(dc), np.zeros_like(dx), np.zeros_like(dxc)] for tn in ("f32", "f64")}

    def split(a, nc):
        return a[0], a[1:1 + nc], a[1 + nc:1 + nc + nd], a[1 + nc + nd:].reshape(nc, nd, n)

    for t, (base, move) in enumerate(results):
        nc = ncs[t]
        v[t], dc[coff[t]:coff[t + 1]], dx[t], dxc[coff[t]:coff[t + 1]] = split(base, nc)
        for tn in sp:
            a, b, c, d = split(move[tn], nc)
            sp[tn][0][t], sp[tn][1][coff[t]:coff[t + 1]], sp[tn][2][t], sp[tn][3][coff[t]:coff[t + 1]] = a, b, c, d
    out.update(v=v, dc=dc, dx=dx, dxc=dxc)
    for tn in sp:
        for name, a in zip(("sv", "sdc", "sdx", "sdxc"), sp[tn]):
            out[f"{tn}/{name}"] = encode(a)
    path = Path(__file__).with_name("deriv_grad_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(all_trees), "trees,", int(coff[-1]), "constants,", path.stat().st_size, "bytes; constants per tree", ncs)


if __name__ == "__main__":
    main()
