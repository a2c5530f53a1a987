"""Shared-subtree columns kept per dataset: a context numbers the
subtrees (slot registry), a dataset keeps the derived columns in a pool, and a
call derives only the columns the pool does not hold under the program's slots.

Every case (tests/column_cache_cases.py) is run here with the pool on and
compared, call by call, with the same calls of a fresh child process run with
SRHIP_COLUMN_CACHE=0, the per-call derive pass: Σ w·ℓ, Σ w and did_succeed must
be bit-identical. The context's counters must be what a model of the pool
(slot -> key, from the programs' own {key: slot}) predicts.

Preconditions are asserted first, so that no case passes by exercising
nothing: both populations have at least 4 shared columns, their key sets
share a key and differ in a key."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import column_cache_cases as cases

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent


@pytest.fixture(scope="module")
def reference(gpu_ctx):
    """Every case once, in a child process, with the pool off."""
    env = dict(os.environ, SRHIP_COLUMN_CACHE="0")
    env.pop("SRHIP_COLUMN_SLOTS", None)
    run = subprocess.run([sys.executable, str(HERE / "column_cache_cases.py")], env=env, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr[-4000:]
    ref = json.loads(run.stdout.strip().splitlines()[-1])
    for name, r in ref.items():  # the reference really is the per-call path: nothing reused, every call derives
        n = 0
        for c in r["calls"]:
            n += len(r["columns"][c["program"]])
            assert c["counters"]["reused"] == 0 and c["counters"]["derived"] == n, (name, c["counters"])
    return ref


def preconditions(columns):
    for name, cols in columns.items():
        print(name, len(cols), "shared columns")
        assert len(cols) >= 4, (name, cols)
        assert len(set(cols.values())) == len(cols), "two keys in one slot"
    if "A" in columns and "B" in columns:
        a, b = set(columns["A"]), set(columns["B"])
        print("A and B:", len(a & b), "A only:", len(a - b), "B only:", len(b - a))
        assert a & b, "the populations share no subtree"
        assert a ^ b, "the populations' subtrees are the same"


def model(calls, columns, fallback=(), new_pool_before=()):
    """(derived, reused, derive programs) after each call: the pool as slot -> key;
    a call in `fallback` derives every column into the per-call buffer."""
    pool, derived, reused, programs, built = {}, 0, 0, 0, {}
    out = []
    for i, c in enumerate(calls):
        cols = columns[c["program"]]
        if i in new_pool_before:
            pool = {}
        if i in fallback:
            miss = sorted(cols)
        else:
            miss = sorted(k for k, s in cols.items() if pool.get(s) != k)
            for k in miss:
                pool[cols[k]] = k
        derived += len(miss)
        reused += len(cols) - len(miss)
        if miss and built.get(c["program"]) != miss:  # a derive program of just those subtrees
            built[c["program"]] = miss
            programs += 1
        out.append(dict(derived=derived, reused=reused, programs=programs))
    return out


def check(name, reference, fallback=(), new_pool_before=()):
    got = cases.CASES[name]()
    ref = reference[name]
    preconditions(got["columns"])
    assert {k: set(v) for k, v in got["columns"].items()} == {k: set(v) for k, v in ref["columns"].items()}, \
        "the pool changes which subtrees are shared"
    assert len(got["calls"]) == len(ref["calls"])
    want = model(got["calls"], got["columns"], fallback, new_pool_before)
    for i, (g, r, w) in enumerate(zip(got["calls"], ref["calls"], want)):
        counters = {k: g["counters"][k] for k in ("derived", "reused", "programs")}
        print(name, "call", i, g["program"], counters, "model", w)
        assert g["tree_code"] > 0 and g["tree_code"] == r["tree_code"]
        assert g["ok"] == r["ok"], f"call {i}: did_succeed differs from the per-call path"
        assert g["sums"] == r["sums"], f"call {i}: loss sums differ from the per-call path"
        assert g["wsum"] == r["wsum"]
        assert counters == w, f"call {i}"
    return got, want


def test_same_program_again_derives_nothing(reference):
    got, want = check("again", reference)
    n = len(got["columns"]["A"])
    assert want[0] == dict(derived=n, reused=0, programs=1)
    assert want[1] == dict(derived=n, reused=n, programs=1)


def test_other_program_derives_only_its_new_subtrees(reference):
    got, want = check("a_then_b", reference)
    a, b = got["columns"]["A"], got["columns"]["B"]
    for k in set(a) & set(b):
        assert a[k] == b[k], "a shared subtree keeps its slot"
    assert want[1]["derived"] - want[0]["derived"] == len(set(b) - set(a))
    assert want[1]["reused"] == len(set(a) & set(b))


def test_displaced_columns_are_derived_again(reference):
    got, want = check("displace", reference)
    assert got["calls"][0]["counters"]["nslot"] == got["nslot"]
    again = want[2]["derived"] - want[1]["derived"]
    print("derived again by A's second call:", again)
    assert again > 0, "B displaced none of A's columns"
    assert got["calls"][0]["sums"] == got["calls"][2]["sums"] and got["calls"][0]["ok"] == got["calls"][2]["ok"]


def test_gathered_rows_take_the_per_call_path(reference):
    got, want = check("row_idx", reference, fallback={1})
    n = len(got["columns"]["A"])
    assert want[2] == dict(derived=2 * n, reused=n, programs=1)  # the pool was left valid
    assert got["calls"][0]["sums"] == got["calls"][2]["sums"]


def test_failing_subtree_fails_its_trees_from_the_pool_too(reference):
    import srhip.constants as K

    got, want = check("failing", reference)
    e = K.UOP["EXP"]
    nested = [k for k in got["columns"]["F"] if k.startswith(f"u{e}(u{e}(u{e}(")]
    print(nested)
    assert nested, "exp(exp(exp(x))) is not a shared column"
    assert want[1]["derived"] == want[0]["derived"], "the second call derived again"
    for c in got["calls"]:
        ok = np.frombuffer(bytes.fromhex(c["ok"]), np.uint8)
        assert not ok[:cases.NFAIL].any(), "a tree reading the failed column succeeded"
        assert ok[cases.NFAIL:].any()


def test_new_dataset_holds_no_stale_column(reference):
    got, want = check("new_dataset", reference, new_pool_before={1})
    n = len(got["columns"]["A"])
    assert want[1] == dict(derived=2 * n, reused=0, programs=1)
    assert got["calls"][0]["sums"] != got["calls"][1]["sums"]  # other X, other losses


def test_program_of_another_context_takes_the_per_call_path(reference):
    got, want = check("two_contexts", reference, fallback={0, 1})
    assert want[1]["reused"] == 0
