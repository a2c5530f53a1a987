"""The tree compilers' allocation limits on the CPU (srhip.engine.jit_compile, no device): every
ladder of tests/tree_code_limit_cases.py compiles exactly up to its literal limit in every compiler
it applies to, the rejected rungs give the expected reason, the machine code of these trees (which
fill the register pools, unlike the random programs of tests/test_jit.py) is what llvm-mc makes of
the text mirror, and the oracle evaluates every tree at every row count the GPU test uses."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import srhip
import tree_code_limit_cases as L
from srhip.engine import jit_compile
from test_jit import LLVM, assemble

CELLS = [pytest.param(f, c, id=f"{f}-{c}") for f in L.FAMILIES for c in L.APPLIES[f]]


def compiled(family, compiler, planted=False, **kw):
    T, ckw = L.COMPILERS[compiler]
    trees = list(L.batch(family)[0])
    if planted:
        trees += L.planted_trees(family, compiler, T)
    flat = srhip.flatten(trees, L.opts(), dtype=T)
    code, text, offs = jit_compile(flat, **ckw, **kw)
    return code, text, sorted(offs)


@pytest.mark.parametrize("family,compiler", CELLS)
def test_ladders_compile_exactly_up_to_their_limits(family, compiler):
    _, _, got = compiled(family, compiler)
    ids = L.batch(family)[1]
    assert got == L.expected(family, compiler), (family, compiler, [ids[t] for t in got])
    for lad, (rungs, _, _) in L.FAMILIES[family].items():  # each literal is a rung of its ladder, or 0
        lim = L.LIMITS[lad][compiler]
        assert lim is L.ALL or lim == 0 or lim in rungs, (lad, compiler, lim)


@pytest.mark.parametrize("compiler", L.GRAD)
def test_long_gradient_program(compiler):
    """4096 program steps (4098 nodes) compile, 4097 are "program too long"."""
    T, ckw = L.COMPILERS[compiler]
    rungs, build = L.LONG
    flat = srhip.flatten([build(r) for r in rungs], L.opts(), dtype=T)
    assert [int(flat.node_off[i + 1] - flat.node_off[i]) for i in range(len(rungs))] == rungs
    _, _, offs = jit_compile(flat, **ckw)
    assert sorted(offs) == [i for i, r in enumerate(rungs) if r <= L.LONG_LIMIT]


@pytest.mark.parametrize("family,compiler", [c for c in CELLS if c.values[0] in L.PLANTED])
def test_planted_copies_of_the_limit_rungs_compile(family, compiler):
    """The failing copies the GPU test plants (limit rung + x1·c) are tree code too."""
    n = len(L.batch(family)[0])
    _, _, got = compiled(family, compiler, planted=True)
    nplant = len(L.limit_rungs(family, compiler))
    assert got == L.expected(family, compiler) + list(range(n, n + nplant)), (family, compiler, got)


_CHILD = r"""
import json, sys
import srhip, tree_code_limit_cases as L
from srhip.engine import jit_compile
for fam in L.FAMILIES:
    for comp in L.APPLIES[fam]:
        T, kw = L.COMPILERS[comp]
        print(f"@@ {fam} {comp}", file=sys.stderr, flush=True)
        jit_compile(srhip.flatten(list(L.batch(fam)[0]), L.opts(), dtype=T), **kw)
for comp in L.GRAD:
    T, kw = L.COMPILERS[comp]
    print(f"@@ long {comp}", file=sys.stderr, flush=True)
    jit_compile(srhip.flatten([L.LONG[1](r) for r in L.LONG[0]], L.opts(), dtype=T), **kw)
"""


@pytest.fixture(scope="module")
def reasons():
    """{(family, compiler): {tree id: reason}} printed by a child process under SRHIP_JIT_DEBUG
    (the switch is read once per process)."""
    env = dict(os.environ, SRHIP_JIT_DEBUG="1", SRHIP_JIT_THREADS="1", PYTHONPATH=os.pathsep.join(sys.path))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out, key = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@ "):
            key = tuple(line.split()[1:])
            out[key] = {}
            continue
        m = re.search(r"tree (\d+) not compiled: (.*)", line)
        if m and key:
            out[key][int(m.group(1))] = m.group(2).strip()
    return out


@pytest.mark.parametrize("family,compiler", CELLS)
def test_rejected_rungs_give_the_expected_reason(reasons, family, compiler):
    ids = L.batch(family)[1]
    want = {t: L.WHY.get(lad, {}).get(compiler, {}).get(r) for t, (lad, r) in enumerate(ids)}
    want = {t: w for t, w in want.items() if w is not None}
    # every rung above a limit that the compiler was offered has a reason in WHY, and no other tree
    got = reasons[(family, compiler)]
    assert got == want, (family, compiler, {ids[t]: w for t, w in got.items()})
    assert set(got).isdisjoint(L.expected(family, compiler))


@pytest.mark.parametrize("compiler", L.GRAD)
def test_long_program_reason(reasons, compiler):
    assert reasons[("long", compiler)] == {2: "program too long"}


@pytest.mark.skipif(not (LLVM / "llvm-mc").exists(), reason="llvm-mc not installed")
@pytest.mark.parametrize("family,compiler", CELLS)
def test_machine_code_equals_llvm_mc(family, compiler):
    code, text, got = compiled(family, compiler)
    assert got and assemble(text) == code, (family, compiler)


@pytest.mark.parametrize("family", ["live-values", "features-held", "constants"])
def test_threaded_layout_equals_serial(family):
    """text=False takes build()'s threaded code generation (provisional addresses, the layout,
    every tree again at its final address): the serial generator's bytes and offsets."""
    for compiler in ("loss32", "loss32p", "memc32", "out32"):
        T, ckw = L.COMPILERS[compiler]
        trees = list(L.batch(family)[0]) * 40  # enough trees for several threads' shares
        flat = srhip.flatten(trees, L.opts(), dtype=T)
        code_t, _, offs_t = jit_compile(flat, **ckw)
        code_p, text_p, offs_p = jit_compile(flat, **ckw, text=False)
        assert text_p == "" and offs_p == offs_t and code_p == code_t, (family, compiler)


def parts_copies():
    """Copies of the parts family's tree that overflow one code area: from len(code) of one tree in
    the 64-byte aligned layout and the area size, plus a margin of 64 trees."""
    flat = srhip.flatten([L.parts_base()], L.opts(), dtype=np.float32)
    code, _, offs = jit_compile(flat)
    assert offs == {0: 0}
    per_tree = -(-len(code) // 64) * 64
    return L.AREA_BYTES // per_tree + 64, per_tree


def test_parts_family_fills_one_code_area():
    """The device-free compiler fills one area and stops (jit::build opens the next part there): the
    copies it takes are the leading ones, the area is full to within one tree, and the threaded
    layout (text=False) gives the serial generator's bytes and offsets on all of them."""
    ncopies, per_tree = parts_copies()
    assert ncopies <= 20000
    P = L.parts_problem(ncopies)
    assert int(P.ok.sum()) == ncopies  # the oracle's success count
    nc = len(P.flat.consts) // ncopies
    assert len({P.flat.consts[j * nc:(j + 1) * nc].tobytes() for j in range(ncopies)}) == ncopies  # distinct constants
    code_p, text_p, offs_p = jit_compile(P.flat, text=False)
    code_t, _, offs_t = jit_compile(P.flat)
    assert text_p == "" and offs_p == offs_t and code_p == code_t
    assert sorted(offs_t) == list(range(len(offs_t))) and len(offs_t) < ncopies
    assert L.AREA_BYTES - 64 - per_tree < len(code_t) <= L.AREA_BYTES - 64
    assert ncopies - len(offs_t) >= 32  # the second part holds more than a handful of trees


@pytest.mark.parametrize("compiler", ["loss32", "loss32p"])
def test_columns_are_kept_up_to_the_pool(compiler):
    """columns-and-pool: with the twelve filler trees (three column loads each) a rung of F features
    reads its four columns up to F = COLS_LIMIT and is its own code, without a global load, beyond."""
    T, ckw = L.COMPILERS[compiler]
    fill = list(L.batch("columns-and-pool", "fill")[0])
    rungs, build, _ = L.FAMILIES["columns-and-pool"]["cols"]
    assert L.COLS_LIMIT in rungs and L.COLS_LIMIT + 1 in rungs
    for F in rungs:
        flat = srhip.flatten(fill + [build(F)], L.opts(), dtype=T)
        _, text, offs = jit_compile(flat, **ckw)
        assert len(offs) == len(fill) + 1
        loads = text.count("global_load_dwordx4")
        assert loads == 3 * len(fill) + (L.NCOLS if F <= L.COLS_LIMIT else 0), (compiler, F, loads)
    for comp in ("memc32", "out32"):  # no columns for memory-constant and per-row output code
        _, text, _ = jit_compile(srhip.flatten(fill, L.opts(), dtype=T), **L.COMPILERS[comp][1])
        assert "global_load_dwordx4" not in text


@pytest.mark.parametrize("family", list(L.FAMILIES))
@pytest.mark.parametrize("T", L.DTYPES, ids=lambda T: np.dtype(T).name)
def test_oracle_evaluates_every_tree(family, T):
    ntrees = len(L.batch(family)[0])
    assert L.oracle_success_counts(family, T) == {n: ntrees for n in L.ROWS}


@pytest.mark.parametrize("family,compiler", [(f, c) for f in ("live-values", "features-held") for c in ("loss32", "loss64", "grad32", "grad64")]
                         + [("wide-window", "wide32")])
def test_oracle_fails_exactly_the_planted_copies(family, compiler):
    P = L.problem(family, L.COMPILERS[compiler][0], L.BIG, planted=compiler)
    assert P.flat.ntrees > P.nfam and P.ok[:P.nfam].all() and not P.ok[P.nfam:].any()
