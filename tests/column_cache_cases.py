"""The scenarios of tests/test_column_cache_gpu.py: sequences of eval_loss calls
whose shared-subtree columns come from a dataset's column pool.

A scenario opens its own contexts (the slot registry and the counters are per
context), runs its calls and returns, per call, the losses' and did_succeed's
bytes and the context's counters after the call, and per program its
{canonical subtree text: slot}. The test runs each scenario in its own process
state with the pool on, and all of them once in a child process with
SRHIP_COLUMN_CACHE=0 (`python column_cache_cases.py`: one JSON object).

Shapes: 320 trees (Float32 tree code needs 256), + - * / cos exp, maxsize 30,
5 features, 3000 rows (three row groups, the last one ragged)."""
import gc
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT / "symbolicregression.jl_amd",):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

NTREES, NFEAT, ROWS = 320, 5, 3000
SEED_A, SEED_B = 1000, 2000
BIN, UN = ["+", "-", "*", "/"], ["cos", "exp"]
NFAIL = 6  # trees holding the overflowing subtree (at least 4, so that it is kept)


def options():
    import srhip

    return srhip.Options(binary_operators=BIN, unary_operators=UN)


def population(seed):
    import srhip

    return srhip.random_population(NTREES, options(), NFEAT, np.float32, seed=seed, maxsize=30)


def data(seed=1):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((NFEAT, ROWS)).astype(np.float32)
    y = (np.float32(2) * np.cos(X[3]) + X[0] * X[0] - np.float32(2)).astype(np.float32)
    return X, y


def failing_population():
    """Population A with NFAIL trees c + exp(exp(exp(x1))) in front: the subtree
    overflows Float32 on the rows where x1 > ~1.5 (exp(exp(1.5)) = 88.4)."""
    import srhip
    from srhip import Node

    o = options()
    eee = lambda: o.make_unary("exp", o.make_unary("exp", o.make_unary("exp", Node(feature=2))))  # noqa: E731
    special = [o.make_binary("+", eee(), Node(val=0.5 + k)) for k in range(NFAIL)]
    return special + population(SEED_A)[NFAIL:]


class Run:
    """One context, its datasets and programs; every call is recorded."""

    def __init__(self, nslot=None):
        import srhip

        old = os.environ.get("SRHIP_COLUMN_SLOTS")
        if nslot is not None:
            os.environ["SRHIP_COLUMN_SLOTS"] = str(nslot)
        try:
            self.ctx = srhip.engine.Context(0)
        finally:
            if nslot is not None:
                if old is None:
                    del os.environ["SRHIP_COLUMN_SLOTS"]
                else:
                    os.environ["SRHIP_COLUMN_SLOTS"] = old
        self.calls = []
        self.columns = {}
        self.keep = []

    def dataset(self, X, y):
        import srhip

        return srhip.engine.DeviceDataset(self.ctx, X, y)

    def program(self, name, trees):
        import srhip

        p = srhip.engine.Program(self.ctx, srhip.flatten(trees, options(), dtype=np.float32), np.float32)
        self.columns[name] = p.shared_columns()
        self.keep.append(p)
        return p

    def call(self, name, p, ds, row_idx=None):
        s, w, ok = p.eval_loss(ds, 0, row_idx=row_idx)
        self.calls.append(dict(program=name, sums=np.asarray(s, np.float64).tobytes().hex(), wsum=float(w),
                               ok=np.asarray(ok, np.uint8).tobytes().hex(), tree_code=self.ctx.last_tree_code(),
                               counters=self.ctx.column_cache_info()))

    def result(self):
        out = dict(calls=self.calls, columns=self.columns)
        self.keep.clear()
        gc.collect()
        self.ctx.close()
        return out


def case_again():
    r = Run()
    ds = r.dataset(*data())
    a = r.program("A", population(SEED_A))
    r.call("A", a, ds)
    r.call("A", a, ds)
    del ds, a
    return r.result()


def case_a_then_b():
    r = Run()
    ds = r.dataset(*data())
    a = r.program("A", population(SEED_A))
    b = r.program("B", population(SEED_B))
    r.call("A", a, ds)
    r.call("B", b, ds)
    del ds, a, b
    return r.result()


def case_displace():
    """As many slots as the larger program has columns: B's own columns displace A's."""
    probe = Run()
    na = len(probe.program("A", population(SEED_A)).shared_columns())
    nb = len(probe.program("B", population(SEED_B)).shared_columns())
    probe.result()
    r = Run(nslot=max(na, nb))
    ds = r.dataset(*data())
    a = r.program("A", population(SEED_A))
    b = r.program("B", population(SEED_B))
    r.call("A", a, ds)
    r.call("B", b, ds)
    r.call("A", a, ds)
    del ds, a, b
    out = r.result()
    out["nslot"] = max(na, nb)
    return out


def case_row_idx():
    r = Run()
    ds = r.dataset(*data())
    a = r.program("A", population(SEED_A))
    idx = np.random.default_rng(3).integers(0, ROWS, 1000)
    r.call("A", a, ds)
    r.call("A", a, ds, row_idx=idx)
    r.call("A", a, ds)
    del ds, a
    return r.result()


def case_failing():
    r = Run()
    X, y = data()
    X[1, 17] = 2.0  # feature 2: exp(exp(exp(2))) overflows whatever the other rows hold
    ds = r.dataset(X, y)
    f = r.program("F", failing_population())
    r.call("F", f, ds)
    r.call("F", f, ds)
    del ds, f
    return r.result()


def case_new_dataset():
    r = Run()
    a = r.program("A", population(SEED_A))
    ds = r.dataset(*data(1))
    r.call("A", a, ds)
    del ds
    gc.collect()  # destroyed: its pool goes with it
    ds = r.dataset(*data(2))
    r.call("A", a, ds)
    del ds, a
    return r.result()


def case_two_contexts():
    """A program of the second context on a dataset of the first."""
    r1, r2 = Run(), Run()
    ds = r1.dataset(*data())
    a = r2.program("A", population(SEED_A))
    r2.call("A", a, ds)
    r2.call("A", a, ds)
    del a
    out = r2.result()
    del ds
    r1.result()
    return out


CASES = dict(again=case_again, a_then_b=case_a_then_b, displace=case_displace, row_idx=case_row_idx,
             failing=case_failing, new_dataset=case_new_dataset, two_contexts=case_two_contexts)


if __name__ == "__main__":
    names = sys.argv[1:] or sorted(CASES)
    print(json.dumps({n: CASES[n]() for n in names}))
