"""Trees built to sit at the tree compilers' allocation limits (csrc/jit.cpp, jit64.cpp,
jit_grad.cpp), for tests/test_tree_code_limits.py (CPU) and test_tree_code_limits_gpu.py.

Each family is a set of ladders; a ladder is a list of integer rungs and a builder, and crosses
one limit of one or more compilers. LIMITS holds, per ladder and compiler, the largest rung that
compiles: every rung up to it compiles and every rung above it is rejected, with the reason in
WHY where the compiler gives one. The limits were found with srhip.engine.jit_compile and are
kept as literals; the comment beside each derives it from the generated layout headers
(csrc/gen/jit_layout_r4.h, jit64_layout.h).

Operators: + - * only (one `/`, in the wide family's planted failing copy; single VALU instructions in tree code, so predictions are bit-exact
against the oracle, as in tests/test_variant_matrix_gpu.py). Features are uniform in
[-1.2, 1.2], constants in ±[0.25, 1], every feature column distinct. Checked on the CPU with
the oracle: every tree of every family succeeds in both dtypes at every n of ROWS (asserted as
exact counts in both test files); on the planted data exactly the planted copies fail.

What a loss or output compiler is offered: trees whose interpreter stack need is at most
kShallowSlots = 2 (srhip_internal.h; api.cpp `candidates`), so a balanced tree of more than
three levels never reaches them and "live values" can fill their pool only together with held
features. The gradient compilers are offered every tree.

The long family is reachable (LONG below: a 4096-step gradient program compiles, 4097 steps do
not) and pinned on the CPU only: its 4095-operation trees are far past the rounding model behind
the Float32 gradient bound of the variant matrix.
"""
import functools
from types import SimpleNamespace

import numpy as np

import oracle
import srhip
from srhip import Node

ADD, SUB, MUL, DIV = 1, 2, 3, 4
LO, HI, PLANT = -1.2, 1.2, 2.4
DTYPES = [np.float32, np.float64]

# rows: 1, around the Float64 tile (64 lanes x 2 rows = 128: jit64.cpp TILE2, gen_jit64.py blocks of
# two doubles) and the Float32 tile (64 lanes x SR_JIT_R = 4 rows = 256, loss, output and gradient
# code alike), and two row groups of which the second is one partial tile
BIG = 8192 + 256 + 1
ROWS = [1, 127, 128, 129, 255, 256, 257, BIG]


@functools.lru_cache(maxsize=None)
def opts():
    return srhip.Options(binary_operators=["+", "-", "*", "/"], unary_operators=["neg", "abs", "square", "cube"])


# the compilers: name -> (dtype, keywords of srhip.engine.jit_compile)
COMPILERS = {
    "loss32": (np.float32, dict()),                        # Float32 loss code, FAST allowed
    "loss32p": (np.float32, dict(fast=False)),             # the same, PRECISE only
    "memc32": (np.float32, dict(memc=True)),               # memory-constant loss code
    "out32": (np.float32, dict(out=True, fast=False)),     # per-row output code
    "wide32": (np.float32, dict(wide=True)),               # features from device memory
    "loss64": (np.float64, dict()),
    "out64": (np.float64, dict(out=True)),
    "grad32": (np.float32, dict(grad=True)),
    "grad64": (np.float64, dict(grad=True)),
}
LOSS_LIKE = ("loss32", "loss32p", "memc32", "out32", "loss64", "out64")
GRAD = ("grad32", "grad64")


def X(f):
    return Node(feature=int(f))


def const(i):
    """Constant number i of a tree: ±[0.25, 1], a fixed sequence."""
    return Node(val=float((0.25 + 0.75 * ((i * 0.381966) % 1.0)) * (-1.0 if i % 3 == 1 else 1.0)))


def _op(i):
    return (ADD, SUB, MUL)[i % 3]


def balanced(leaves):
    lv, k = list(leaves), 0
    while len(lv) > 1:
        lv = [Node(_op(k + i), lv[2 * i], lv[2 * i + 1]) for i in range(len(lv) // 2)]
        k += 1
    return lv[0]


def reread(t, F, f0=1):
    """t ∘ x_f0 ∘ ... ∘ x_(f0+F-1): every one of the F features is read once more, last."""
    for f in range(f0, f0 + F):
        t = Node((MUL, ADD, SUB)[f % 3], t, X(f))
    return t


def bal_held(depth, F):
    """`depth` levels over 2^depth leaves that cycle through x1..xF (the first and the last leaf are
    constants), then every feature again: at the peak F feature blocks and `depth` values are live."""
    n = 2 ** depth
    leaves = [const(i) if i in (0, n - 1) else X(i % F + 1) for i in range(n)]
    return reread(balanced(leaves), F)


def right_comb(n):
    """x1 ∘ (x2 ∘ (... (xn ∘ c))): n features read before the first operation completes."""
    t = Node(MUL, X(n), const(n))
    for f in range(n - 1, 0, -1):
        t = Node(_op(f), X(f), t)
    return t


def held(F, f0=1):
    """x_f0·c, then x_(f0+1) .. x_(f0+F-1) read for the first time, then all F again: F features held
    across the whole tree and one running value."""
    t = Node(MUL, X(f0), const(F))
    for f in range(f0 + 1, f0 + F):
        t = Node((ADD, SUB)[f % 2], t, X(f))
    return reread(t, F, f0)


def high(f):
    """(x_f·c + x_1)·x_f: feature f (1-based) read by an inline operator, twice."""
    return Node(MUL, Node(ADD, Node(MUL, X(f), const(f)), X(1)), X(f))


def const_terms(k):
    """((x1·c0 + c1)·c2 + c3) ...: exactly k constants, each an operand of the running value (nothing
    folds), a feature subtracted at every third step; at most 63 interpreter instructions, so the
    loss compilers are offered it (srhip_internal.h kVProgMax)."""
    t = Node(MUL, X(1), const(0))
    for i in range(1, k):
        t = Node(ADD if i % 2 else MUL, t, const(i))
        if i % 3 == 0:
            t = Node(SUB, t, X(i % 5 + 1))
    return t


def long_tree(nodes):
    """A balanced tree of 4095 nodes over x1..x4 and two constants, under `nodes - 4095` negations."""
    t = balanced([const(i) if i in (0, 1024) else X(i % 4 + 1) for i in range(2048)])
    for _ in range(nodes - 4095):
        t = Node(1, t)  # neg
    return t


NCOLS = 4  # shared-subtree columns of the columns-and-pool family


def quotient(k):
    """x_k / x_(k+4), k = 1..4: constant-free subtrees with a routine, shared by every tree of the
    family, so each becomes a shared-subtree column (jit.cpp plan_shared). Both operands are features
    of the dataset, |x| <= 1.2 and (at these seeds) >= 2^-45: the packed division's IEEE-exact range
    (tests/test_jit_gpu.py test_variable_divisor_is_ieee_exact)."""
    return Node(DIV, X(k), X(k + NCOLS))


def cols_held(F):
    """The four columns, then F raw features x9.., then all of them again: 4 + F preloaded blocks
    held across the tree, and the running value."""
    t = Node(MUL, quotient(1), const(F))
    for k in range(2, NCOLS + 1):
        t = Node((ADD, SUB)[k % 2], t, quotient(k))
    for f in range(9, 9 + F):
        t = Node((ADD, SUB)[f % 2], t, X(f))
    for k in range(1, NCOLS + 1):
        t = Node((ADD, SUB, MUL)[k % 3], t, quotient(k))
    return reread(t, F, 9)


def cols_filler(j):
    """q_a·c + (q_b − q_c): small trees that read three of the columns each."""
    a, b, c = (j % NCOLS + 1, (j + 1) % NCOLS + 1, (j + 2) % NCOLS + 1)
    return Node(ADD, Node(MUL, quotient(a), const(j)), Node(SUB, quotient(b), quotient(c)))


# family -> {ladder: (rungs, builder, features of its dataset)}
FAMILIES = {
    "live-values": {
        "bal3": ([3, 4, 5, 6, 7], lambda F: bal_held(3, F), 21),
        "bal4": ([13, 14, 15, 16, 17, 18], lambda F: bal_held(4, F), 21),
        "comb": ([7, 8, 9, 19, 20, 21], right_comb, 21),
    },
    "features-held": {
        "held": ([6, 7, 8, 9, 18, 19, 20, 21], held, 21),
        "root": ([3], lambda f: X(f), 21),                      # a feature as the root
        "same": ([2], lambda f: Node(MUL, X(f), X(f)), 21),     # both operands the same feature
    },
    "high-features": {
        "high63": ([61, 62, 63], high, 63),
        "high64": ([61, 62, 63, 64], high, 64),
        "high78": ([61, 62, 63, 64, 78], high, 78),
    },
    "constants": {
        "const": ([15, 16, 17], const_terms, 5),
    },
    "wide-window": {
        "wide": ([2, 3, 4, 5, 6, 7, 8, 9], lambda k: held(k, 64), 160),
    },
    "columns-and-pool": {
        "cols": ([1, 2, 3, 4, 5], cols_held, 14),
        "fill": (list(range(1, 13)), cols_filler, 14),
    },
}
LONG = ([4097, 4098, 4099], long_tree)  # nodes; gradient compilers, CPU test only

ALL = object()  # marker: every rung of the ladder compiles


def _all(*names):
    return {c: ALL for c in names}


# The largest rung that compiles, per ladder and compiler (0: none does).
LIMITS = {
    # SR_JIT_V_NPOOL = SR_JIT64_V_NPOOL = 8 blocks: F held features + 3 live values of the three
    # levels, F <= 5. SR_JIT_G_GNPOOL = SR_JIT64_G_NPOOL = 20: every rung fits.
    "bal3": {**{c: 5 for c in LOSS_LIKE}, "wide32": 5, **_all(*GRAD)},
    # four levels need 3 interpreter slots: never offered to the loss / output compilers.
    # Gradient pool: F held features + 4 live values + the adjoint block that the reverse pass needs as
    # soon as the tree holds a constant (the adjoints share the pool) <= 20, so F <= 15; the same tree
    # without its two constant leaves compiles at F = 16.
    "bal4": {**{c: 0 for c in LOSS_LIKE}, "wide32": 0, "grad32": 15, "grad64": 15},
    # n features preloaded before the first operation: n <= NPOOL (8, gradient 20); the first
    # operation frees two. Wide code loads through its window and takes every rung.
    "comb": {**{c: 8 for c in LOSS_LIKE}, "wide32": ALL, "grad32": 20, "grad64": 20},
    # F held features + the running value: F + 1 <= NPOOL, so 7 and 19.
    "held": {**{c: 7 for c in LOSS_LIKE}, "wide32": 7, "grad32": 19, "grad64": 19},
    "root": _all(*LOSS_LIKE, "wide32", *GRAD),
    "same": _all(*LOSS_LIKE, "wide32", *GRAD),
    # (1 + f0)·TILE·4 + 3·4·64 <= 65535 with TILE = 256 and f0 the 0-based index: f0 <= 62, the
    # 63rd feature; the Float64 compilers test f0 > 62 directly. Wide code has no such bound.
    "high63": _all(*LOSS_LIKE, "wide32", *GRAD),
    "high64": {**{c: 63 for c in LOSS_LIKE + GRAD}, "wide32": ALL},
    "high78": {**{c: 63 for c in LOSS_LIKE + GRAD}, "wide32": ALL},
    # SR_JIT_G_NGACC = SR_JIT64_G_NACC = 16 accumulators, one per constant; memory-constant code
    # holds constants in NSC = 16 SGPRs (jit.cpp Gen::NSC); literal-constant code has no bound.
    "const": {**_all("loss32", "loss32p", "out32", "wide32", "loss64", "out64"), "memc32": 16, "grad32": 16,
              "grad64": 16},
    # k held features + the running value in 8 blocks: k <= 7, as the LDS code's "held"
    "wide": {"wide32": 7},
    # every rung compiles: a tree whose columns and features do not fit is compiled again without
    # columns (jit.cpp gen_tree's second attempt); COLS_LIMIT says which rungs keep their columns
    "cols": _all(*LOSS_LIKE, *GRAD),
    "fill": _all(*LOSS_LIKE, *GRAD),
}
# columns-and-pool, Float32 loss code: 4 column blocks + F feature blocks + the running value
# <= SR_JIT_V_NPOOL = 8, so up to F = 3 a rung reads its four columns (four global loads); from
# F = 4 on it is its own code, with no global load.
COLS_LIMIT = 3
# jit_grad.cpp / jit64.cpp: pc > 4096 is "program too long". The two constant leaves are immediates
# of their operators' instructions, not steps of their own: 4098 nodes are 4096 steps.
LONG_LIMIT = 4098

# The reason a rejected rung prints under SRHIP_JIT_DEBUG (rungs not offered print none).
_POOL, _FEAT, _DS = "register pool exhausted", "more features than register blocks", "feature offset beyond the DS immediate"
WHY = {
    "bal3": {**{c: {6: _POOL, 7: _POOL} for c in LOSS_LIKE}, "wide32": {6: _POOL, 7: _POOL}},
    "bal4": {c: {16: _POOL, 17: _POOL, 18: _POOL} for c in GRAD},
    "comb": {**{c: {9: _FEAT, 19: _FEAT, 20: _FEAT, 21: _FEAT} for c in LOSS_LIKE}, **{c: {21: _FEAT} for c in GRAD}},
    "held": {**{c: {8: _POOL, 9: _FEAT, 18: _FEAT, 19: _FEAT, 20: _FEAT, 21: _FEAT} for c in LOSS_LIKE},
             "wide32": {k: _POOL + " (feature window)" for k in (8, 9, 18, 19, 20, 21)},
             **{c: {20: _POOL, 21: _FEAT} for c in GRAD}},
    "high64": {c: {64: _DS} for c in LOSS_LIKE + GRAD},
    "high78": {c: {64: _DS, 78: _DS} for c in LOSS_LIKE + GRAD},
    "const": {"memc32": {17: "more constants than memory-constant SGPRs"},
              **{c: {17: "more constants than accumulators"} for c in GRAD}},
    "wide": {"wide32": {8: _POOL + " (feature window)", 9: _POOL + " (feature window)"}},
}

# the compilers a family is built for (the wide family's trees read features from index 63 on, which
# every other compiler refuses outright)
APPLIES = {
    "live-values": LOSS_LIKE + ("wide32",) + GRAD,
    "features-held": LOSS_LIKE + ("wide32",) + GRAD,
    "high-features": LOSS_LIKE + ("wide32",) + GRAD,
    "constants": LOSS_LIKE + ("wide32",) + GRAD,
    "wide-window": ("wide32",),
    "columns-and-pool": LOSS_LIKE + GRAD,
}


def limit(ladder, compiler):
    rungs = FAMILIES_BY_LADDER[ladder][0]
    lim = LIMITS[ladder][compiler]
    return max(rungs) if lim is ALL else lim


FAMILIES_BY_LADDER = {lad: spec for fam in FAMILIES.values() for lad, spec in fam.items()}


@functools.lru_cache(maxsize=None)
def batch(family, ladder=None):
    """(trees, [(ladder, rung)] per tree) of a family, or of one of its ladders."""
    trees, ids = [], []
    for lad, (rungs, build, _) in FAMILIES[family].items():
        if ladder in (None, lad):
            for r in rungs:
                trees.append(build(r))
                ids.append((lad, r))
    return trees, ids


def expected(family, compiler, ladder=None):
    """Tree ids of batch(family, ladder) that `compiler` compiles."""
    _, ids = batch(family, ladder)
    return [t for t, (lad, r) in enumerate(ids) if r <= limit(lad, compiler)]


PLANTED = ("live-values", "features-held", "wide-window")  # the families the failure test plants in


def limit_rungs(family, compiler):
    """Tree ids of the limit rungs (the largest compiling one of each ladder that has a rejected rung)."""
    _, ids = batch(family)
    return [t for t, (lad, r) in enumerate(ids)
            if r == limit(lad, compiler) and r < max(FAMILIES_BY_LADDER[lad][0])]


def nfeat(family, ladder=None):
    return max(nf for lad, (_, _, nf) in FAMILIES[family].items() if ladder in (None, lad))


def planted_trees(family, compiler, T):
    """Copies of the family's limit rungs plus x1·c, c = max(T)/2: finite at |x1| <= 1.2, not at 2.4.
    Wide code: plus x1·c / (x64·x64 + 2) (a divisor in [2, 3.44]). The division is the one routine
    operator of these families: it gives the copy a guarded FAST path, without which no tile is ever
    redone PRECISE and the window never restarts; the copy fails, so its value is compared nowhere."""
    trees, _ = batch(family)
    c = float(np.finfo(T).max) / 2
    if compiler == "wide32":
        div = Node(ADD, Node(MUL, X(64), X(64)), Node(val=2.0))
        return [Node(ADD, trees[t].copy(), Node(DIV, Node(MUL, X(1), Node(val=c)), div)) for t in limit_rungs(family, compiler)]
    return [Node(ADD, trees[t].copy(), Node(MUL, X(1), Node(val=c))) for t in limit_rungs(family, compiler)]


@functools.lru_cache(maxsize=None)
def problem(family, T, n, ladder=None, planted=None):
    """The batch on n rows with the oracle's outputs and ∂ŷ/∂c in T (computed once, read-only), in
    the shape check_loss_sums / check_loss_grads of tests/test_variant_matrix_gpu.py read.
    planted: a compiler name; its planted_trees are appended and x1 is 2.4 in the last row."""
    T = np.dtype(T).type
    trees = list(batch(family, ladder)[0])
    nfam = len(trees)
    if planted:
        trees += planted_trees(family, planted, T)
    flat = srhip.flatten(trees, opts(), dtype=T)
    nf = nfeat(family, ladder)
    rng = np.random.default_rng(4000 + 7 * nf + n)
    X_ = rng.uniform(LO, HI, (nf, n))
    if planted:
        X_[0, n - 1] = PLANT  # the last valid row of the second row group
    X_ = X_.astype(T)
    assert len({c.tobytes() for c in X_}) == nf or n < 3  # every feature column distinct
    y = (2 * np.cos(X_[min(3, nf - 1)]) + X_[0] * X_[0] - 2).astype(T)
    ym = np.where(y >= 0, 1, -1).astype(T)
    w = np.abs(rng.standard_normal(n)).astype(T)
    with np.errstate(all="ignore"):
        yhat, ok = oracle.eval_trees(flat, X_, dtype=T)
        grads = {}
        for t in np.flatnonzero(ok):
            k, ar, c = flat.tree(t)
            if len(c) == 0:
                grads[int(t)] = np.zeros((0, n))
                continue
            yh, gc, okt = oracle.eval_grad_consts(k, ar, c.astype(T), X_, len(c), dtype=T)
            assert okt and np.array_equal(yh, yhat[t])
            grads[int(t)] = gc.astype(np.float64)
    for a in (X_, y, ym, w, yhat, ok):
        a.setflags(write=False)
    return SimpleNamespace(name=family, T=T, n=n, nfam=nfam, trees=trees, flat=flat, X=X_, y=y, ym=ym, w=w,
                           yhat=yhat, ok=ok, grads=grads)


def oracle_success_counts(family, T):
    """{n: trees the oracle evaluates without failure}: every tree, at every n of ROWS."""
    return {n: int(problem(family, T, n).ok.sum()) for n in ROWS}


# ---- parts: a program whose code needs a second part ---------------------------------------------
AREA_BYTES = 2097152 * 4  # the large template's code area (csrc/Makefile SR_JIT_AREA_WORDS)
PARTS_ROWS = 300


def parts_base():
    """The largest live-values rung that the Float32 loss code compiles."""
    return bal_held(3, LIMITS["bal3"]["loss32"])


def _scaled(t, j):
    """A copy of t with every constant scaled by 1 - j·2^-16 (distinct per copy, still in ±[0.25, 1))."""
    c = t.copy()
    stack = [c]
    while stack:
        n = stack.pop()
        if n.degree == 0:
            if n.constant:
                n.val = float(np.float32(n.val * (1.0 - j * 2.0 ** -16)))
            continue
        stack.append(n.l)
        if n.degree == 2:
            stack.append(n.r)
    return c


@functools.lru_cache(maxsize=None)
def parts_problem(ncopies):
    """`ncopies` copies of parts_base() with distinct constants on PARTS_ROWS rows, and the oracle's
    outputs (no gradients: the family is loss and output code)."""
    T = np.float32
    base = parts_base()
    trees = [_scaled(base, j) for j in range(ncopies)]
    flat = srhip.flatten(trees, opts(), dtype=T)
    rng = np.random.default_rng(4300)
    X_ = rng.uniform(LO, HI, (21, PARTS_ROWS)).astype(T)
    y = (2 * np.cos(X_[3]) + X_[0] * X_[0] - 2).astype(T)
    ym = np.where(y >= 0, 1, -1).astype(T)
    w = np.abs(rng.standard_normal(PARTS_ROWS)).astype(T)
    with np.errstate(all="ignore"):
        yhat, ok = oracle.eval_trees(flat, X_, dtype=T)
    for a in (X_, y, ym, w, yhat, ok):
        a.setflags(write=False)
    return SimpleNamespace(name="parts", T=T, n=PARTS_ROWS, nfam=ncopies, trees=trees, flat=flat, X=X_, y=y, ym=ym,
                           w=w, yhat=yhat, ok=ok, grads={})
